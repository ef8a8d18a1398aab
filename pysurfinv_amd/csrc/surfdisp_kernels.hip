// surfdisp_kernels.hip -- hand-written HIP kernels for gfx950 (MI355X, CDNA4).
//
// Batched surface-wave dispersion forward solver: the GPU counterpart of the reference's
// fast_surf() path (001cat/pySurfInv fast_surf_src/{fast_surf,init,calcul,flat1,surfa}.f).
// This is NOT a translation of the Fortran: the work decomposition, data layout and the
// root-refinement scheme are designed for 64-wide wavefronts; the reference is cited where a
// formula or a semantic rule is taken from it.
//
// Pipeline for one (batch, wave type):
//   K0 surfdisp_prep_kernel   : AoS model[B][5][L] -> SoA mdl[9][L][B] and / or rows[B][9][L]; per-layer earth-flattening
//                               factors computed ONCE per stack (flat1.f:33-69 recomputes them
//                               40x per solve), validation.
//   K1 surfdisp_phase_kernel  : phase velocities.  A TEAM of G lanes (G = 1..64, one wavefront holds
//                               64/G teams) owns one stack; its period-dependent working stack
//                               (b, rho, d, 1/a^2, 1/b^2 and one derived value per layer) lives in LDS; every loop
//                               iteration each lane evaluates the secular function at its own trial
//                               velocity with the 5-component (Rayleigh) or 2-component (Love)
//                               recursion state in registers.  Periods are walked in order inside the
//                               team (faithful start rule c1 = 0.9*c(k-1), mmax carry-over, failure
//                               guards, NaN semantics: calcul.f:104-220).  Template flags: INDEP (one
//                               team per (stack, period), SURFDISP_INDEPENDENT), FAST (count-guided coarse
//                               scan: Love's default, Rayleigh's opt-in SURFDISP_FASTSCAN), EXACT (the fallback instantiation that restates
//                               DLTAR4 / DLTAR1 / NEVILL statement by statement for the stacks the
//                               production arithmetic cannot treat faithfully); phase-only calls skip
//                               the ellipticity recursions.  The teams of a wavefront run in LOCK STEP: all
//                               scan, then all refine, then all end their period (ST_WREF / ST_WEND).
//   K1b surfdisp_ellip_kernel : Rayleigh ellipticities of teams of >= 4 lanes, one lane per (stack, period),
//                               replaying the working stack's history the root search recorded.
//   K2 surfdisp_group_kernel  : group velocities, one lane per (stack, period): eigenfunction
//                               integration + energy integrals (surfa.f:714-1192 / 374-606), fp64 state
//                               for Rayleigh as in the reference (surfa.f:717-722); the KERN
//                               instantiation also writes the analytic partials dc/d(Vs, Vp, rho).
//   K2e surfdisp_thickness_kernel (surfdisp_forward_thickness_kernels_device only): dc/d(layer thickness, interface depth) from
//                               the layer-top eigenfunctions of the EIG instantiation and the partials' scratch (see K2e below).
//   K3 surfdisp_finish_kernel : period-major internal results -> the caller's [B][P] arrays.
//   K4 (surfdisp_forward_group_kernels_device only) surfdisp_shift_kernel + K2 + surfdisp_group_combine_kernel: roots at
//                               T (1 -+ d) from the first-order prediction, the phase partials there, and the analytic
//                               group-velocity partials formed from them (see K4 below).
// No MFMA: the products are 5x5 / 4x4 / 2x2.  Algorithmic HBM traffic is one read of the model array and one
// write of c/U (the staged copies and period-major intermediates make it 138 MB per 65 536-stack batch against
// 24 MB); everything else is VALU + transcendental work.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <atomic>
#include "surfdisp_internal.h"

#include "surfdisp_k_common.h"
#include "surfdisp_k_prep.h"
#include "surfdisp_k_secular.h"
#include "surfdisp_k_scan.h"
#include "surfdisp_k_rows.h"

namespace sd {

// ================================================================================== K1: phase
// ST_WREF / ST_WEND (lock step, see PhaseArgs::lockstep): a team that has its bracket / its root waits for the other teams
// of its wavefront, so that the refine pass and the end-of-period block run ONCE per period for all of them
// ST_NEVILL0 (Love, production kernel): the pass before NEVILL's first in which the bracket's two end values are evaluated again with
// the reference's arithmetic (see the evaluation block)
enum { ST_SCAN = 0, ST_REFINE = 1, ST_ELLIP = 2, ST_DONE = 3, ST_NEVILL = 4, ST_WREF = 5, ST_WEND = 6, ST_NEVILL0 = 7 };


// INDEP = false: "faithful" - a team owns a stack and walks its periods in order (reference
//   semantics: start rule 0.9*c(k-1), mmax carry-over, failure cascade).
// INDEP = true : "independent" - a team owns ONE (stack, period) root search (BASELINE north_star's
//   work unit): every period starts from the k=1 rule of fast_surf.f:157-171 evaluated at its own
//   period, on a freshly built full stack.  P times more teams, P times shorter dependency chain:
//   the mode for small batches; equal to the faithful mode to ~1e-6 on well-behaved (monotone)
//   stacks, NOT on rough ones (defects 2 and 9) - the caller opts in.
// FAST = true: the count-guided coarse-to-fine scan (Love's default, Rayleigh's opt-in SURFDISP_FASTSCAN; instantiated for
// teams of 2, 4 and 8 lanes only); FAST = false: every grid point, as the reference - the default, and all larger teams.
// EXACT = false: the production root search - factorised Rayleigh recursion, team subdivision + interpolation
//   instead of NEVILL.  Two things those cannot reproduce faithfully:
//   * a bracket with more than one visible sign change - which of several roots NEVILL lands on depends on its
//     evaluation sequence: the team then runs a statement-by-statement NEVILL (surfa.f:2-83, state ST_NEVILL: one
//     evaluation per pass, every lane of the team at the same trial velocity) for that period;
//   * a secular function that leaves the fp32 range - the reference's overflow points depend on how it forms
//     its matrix entries: the team appends its stack to A.fb_list and stops.
// EXACT = true : the fallback that re-solves the listed stacks from their first period with the reference's own
//   matrix-entry arithmetic (delta_rayleigh<false>) and NEVILL for every root.  Only stacks that overflow fp32 get
//   here (physical models never do), so its speed does not matter; launched after the production kernel with a
//   grid for the worst case, idle blocks exit at once.
template <int KIND, int G, bool INDEP, bool FAST = false, bool EXACT = false>
__device__ __forceinline__ void phase_body(const PhaseArgs &A)
{
    extern __shared__ float w_lds[];
    constexpr int S = SD_PHASE_BLOCK / G;                 // stacks (teams) per workgroup
    constexpr int NFK = (KIND == 1) ? NFW_LOVE : NFW;     // fields per layer of the working stack
    constexpr int LS = lds_ls(S, NFK);                    // ... and its layer stride (words)
    const int tid = threadIdx.x;
#ifdef SD_WAVECLOCK
    const unsigned long long wclk0 = __builtin_amdgcn_s_memrealtime();
    // shader cycles (s_memtime) of this wavefront: whole loop, evaluations of the secular function, stack rebuilds
    const unsigned long long wcyc0 = __builtin_readcyclecounter();
    unsigned long long wcyc_eval = 0, wcyc_build = 0, wcyc_pre = 0, wpasses = 0;
    // ... and inside the Rayleigh evaluation (head, layer loop, closure), the lean scan pass's decision block, lean passes
    unsigned long long wsec[3] = {0, 0, 0}, wcyc_lean = 0, wn_lean = 0, wn_double = 0;   // (wn_double: lean passes of two rounds)
    // team-passes by state, layers stepped per pass (the wavefront's trip count = max over lanes) and summed over lanes
    unsigned long long wn_scan = 0, wn_refine = 0, wn_nevill = 0, wn_ellip = 0, wn_idle = 0, wtrip = 0, wlanelayers = 0, wlanes = 0;
#endif
    const int lane = tid & 63;
    const int slot = tid / G;
    const int j = tid % G;                     // lane index inside the team
    const int tbase = lane - j;                // first lane of my team within the wavefront
    const unsigned long long tmask =
        (G == 64) ? ~0ull : (((1ull << (G & 63)) - 1ull) << tbase);
    const int Lcap = A.Lmax, B = A.B, P = A.P;
    long tg = (long)blockIdx.x * S + slot;                 // team index
    bool team_valid = INDEP ? (tg < (long)B * P) : (tg < B);
    if (EXACT) {                                           // the units listed by the production kernel
        team_valid = tg < (long)(*A.fb_count);
        tg = team_valid ? (long)A.fb_list[tg] : 0;
    }
    const int b = INDEP ? (int)(tg % B) : (int)tg;         // consecutive teams = consecutive stacks
    const int k_own = INDEP ? (int)(tg / B) : 0;           // INDEP: the one period this team solves
    float *wq = w_lds + slot;
    // the ellipticity (two more recursions per period, surfa.f:360-363) only feeds the group-velocity
    // kernel: a phase-only call (A.ratio == nullptr) skips it altogether
    // Production teams of >= 4 lanes never compute them: surfdisp_ellip_kernel does (one lane per (stack, period)), and
    // their instantiations carry no ellipticity state at all.  In-kernel: the exact fallback and two-lane teams (an
    // ellipticity pass with both lanes busy).
    constexpr bool ELL_HERE = EXACT || (G < 4);
    const bool want_ratio = ELL_HERE && (KIND == 2) && (A.ratio != nullptr);
    // What is left of two removed arrangements - OVERLAP / ell_pend / js / had_ell (r02: ellipticity passes riding in the next
    // period's first scan pass, a snapshot in a second LDS slot) and q0* / p0phi / back0 (r01: the heuristic coarse scan's
    // look-back) - is constant or never read.  The compiler folds it away, but deleting these statements changes what it
    // generates for up to 48 instantiations (profiles/variants_removed/README.md): they go with the next counter pass.
    constexpr bool OVERLAP = false;
    // NEVILL's interpolation table x(1..11), y(1..11) (surfa.f:8) of this team, behind the working stacks (A.overlap is 0)
    float *nvx = w_lds + (size_t)((!EXACT && G >= 4 && A.overlap != 0) ? 2 : 1) * LS * Lcap + (size_t)slot * 24, *nvy = nvx + 12;
    // staged fields of this team's stack (SoA copy or rows, see PhaseArgs): field f of layer i at M_AT(f, i)
    const float *__restrict__ mrow = A.msrc + (size_t)b * A.ms_b;
    const size_t msf = (size_t)A.ms_f, msi = (size_t)A.ms_i;
#define M_AT(f, i) mrow[(size_t)(f) * msf + (size_t)(i) * msi]

    int n = 0, st = ST_DONE;
    if (team_valid) { n = A.nl[b]; if (n >= 2) st = ST_SCAN; }

    // team-uniform state
    int k = k_own, nsolved = 0, mm_carry = n, mm_frozen = n, sub = 0, passes = 0;
    int nflat_cur = n;                 // layers the current period's rebuild refreshed (recorded for the ellipticity kernel)
    float T = 1.0f, b1top = 0.0f;
    float p0c = 0.0f, p0d = 0.0f;      // "previous point" of lane 0: scan carry or bracket low end
    float cb = 0.0f, db = 0.0f;        // bracket high end (refine)
    float croot = 0.0f, r12 = 0.0f;
    int p0mm = 0;                      // effective half space the value p0d was computed with
    bool p0ok = false;                 // p0d was computed with mm_frozen (usable for interpolation)
    bool first = true;
    int status = SURFDISP_OK;
    // coarse scan (teams of 2..8 lanes): a coarse pass advances FSTRIDE grid points per lane; an interval between two coarse
    // points is skipped only if the mode counts at its ends certify it (see below), otherwise its fine points are scanned
    // as usual
    constexpr int FSTRIDE = (FAST && G <= 4) ? SD_CERT_STRIDE : 4;
    // CERT (Love): the coarse scan's certificate is a theorem IN EXACT ARITHMETIC behind fp32
    // guards - the "unsafe count" tests - whose margins are soaked, not proved.  At fixed frequency the angle of
    // the pair (displacement, stress) at the surface, followed continuously up from the half space, falls monotonically as
    // the trial velocity rises (Sturm / Pruefer), and a mode sits wherever it passes a multiple of pi: the number of modes
    // between two trial velocities is the difference of their crossing counts (delta_love<true>; checked against brute-force
    // root counts on 120 000 random pairs).  Two coarse points with EQUAL counts, the same effective half space (layer
    // dropping is monotone in c) and both below the half-space velocity have no root - hence no sign change at any grid
    // point - between them: the points in between need not be evaluated, and the bracket the point-by-point scan finds is
    // the one this scan finds.  An unsafe count (a sign or a multiple of pi within rounding) fails the certificate.
    // Teams of up to 8 lanes (stacks of up to ~30 layers): 65 536 x L10 0.71 -> 0.48 ms, 65 536 x L30 1.61 -> 1.05 ms; with 16
    // lanes (deep stacks) one plain pass already covers 16 grid points and the coarse pass's dearer evaluations ate the
    // gain (16 384 x L64: 1.12 -> 1.21 ms), so they keep the plain scan.  Checked against the point-by-point scan bit for
    // bit on 5.7e8 random stacks (scripts/soak_cert.py).
    // (Rayleigh: the FAST instantiations are opt-in - SURFDISP_FASTSCAN - and run the same coarse scan on the count of ray_step /
    // ray_close, which is exact but not monotone along the scan line where a branch has a zero-group-velocity point: see there.)
    static_assert(!(FAST && EXACT), "the exact fallback walks every grid point");
    constexpr bool CERT = FAST && (G >= 2) && (G <= 8);
    int p0Kp = 0x40000000;             // Sturm count at p0 (CERT), packed: count + 4096, bit 30 = unsafe
    bool coarse = false;               // this pass scans on the coarse grid
    int fine_left = 1;                 // fine points still to scan before going (back) to coarse
    float q0c = 0.0f, q0d = 0.0f; int q0mm = 0; [[maybe_unused]] bool q0ok = false;   // (left over, see OVERLAP)
    [[maybe_unused]] float p0phi = 0.0f;
    bool ell_pend = false;
    // NEVILL's state between two evaluations (c1, del1 = p0c, p0d; c2, del2 = cb, db; c3 = croot)
    int nv_nev = 1, nv_m = 1, nv_ic = 0;
    bool defer = false;                // !EXACT: this stack goes to the exact fallback kernel
    bool ell_flag = false;             // in-kernel ellipticity of the period at hand: to be redone by the ellipticity kernel
    // ... whenever c^2 is below this: 2 b^2 / c^2 of the stack's fastest layer beyond A.ell_gmax (read once: the prep kernel's statistic)
    const float ell_c2min = (want_ratio && !EXACT && team_valid && A.ovf != nullptr && A.ell_ambig != 0.0f)
                                ? __expf(0.25f * A.ovf[2 * (size_t)B + b]) / A.ell_gmax : 0.0f;

    // (re)build the working stack for period k over the first nflat layers only -- the reference
    // refreshes just the layers inside the previous period's effective half space and leaves the
    // deeper ones stale (calcul.f:112,133); LDS keeps them across periods exactly like COMMON /d/.
    auto build = [&](int nflat) {
        const float lnT = logf(1.0f / T);                      // alog(t_base/t1), calcul.f:122
        for (int i = j; i < nflat; i += G) {
            // only the fields this layer's role needs (regular: dif, qqq, dflat; half space: hsf, hsr);
            // this block runs whenever ANY team of the wavefront changes period, i.e. almost every
            // pass and with one or two teams active, so its loads and divisions are worth counting
            const bool hs = (i == nflat - 1);
            LayerRaw r;
            r.a_ref = M_AT(F_VP, i); r.b_ref = M_AT(F_VS, i); r.rho_ref = M_AT(F_RHO, i);
            r.qs = M_AT(F_QS, i);
            r.dif = hs ? 0.0f : M_AT(F_DIF, i); r.qqq = hs ? 0.0f : M_AT(F_QQQ, i);
            r.dfl = hs ? 0.0f : M_AT(F_DFL, i);
            r.hsf = hs ? M_AT(F_HSF, i) : 0.0f; r.hsr = hs ? M_AT(F_HSR, i) : 0.0f;
            const LayerV v = layer_derive(r, lnT, hs);
            // the reciprocals are this kernel's own helper values (not the reference's): v_rcp + one Newton
            // step (<= 1 ulp) instead of three IEEE divisions
            W_B(i) = v.b; W_R(i) = v.rho; W_D(i) = v.d;
            if (KIND == 1 && !EXACT) W_IR(i) = wk_ilove(v.rho, v.b);             // Love, production: 1/(rho b^2)
            else if (i == 0 || EXACT) W_IR(i) = wk_irho(v.rho);
            if (KIND == 2) {
                W_IA2(i) = EXACT ? v.a : wk_ia2(v.a);                             // exact kernel: a itself (delta_rayleigh_ref)
                W_IB2(i) = wk_ib2(v.b);
            }
        }
        if (KIND == 2 && !EXACT) {
            // the carried state of delta_rayleigh is rescaled by rho(m-1)/rho(m) on entering layer m: formed here, once
            // per period, from the densities now in the slot - the first stale layer below the refreshed ones included
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int top = nflat < n ? nflat : n - 1;
            for (int i = 1 + j; i <= top; i += G) W_IR(i) = wk_rat(W_R(i - 1), W_R(i));
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };

    // growth of the vertical phase between two trial velocities over the first mm - 1 layers of the working stack (see the
    // bracket branch of the scan); every lane of the team calls it.  Returns 0 where two bounds already show it below
    // A.phimulti: no layer's share exceeds omega d sqrt(1/c1^2 - 1/c2^2) per wave type (sqrt(x + e) - sqrt(x) <= sqrt(e)) and only
    // layers that are oscillatory at c2 have one - first with the thickness of the whole working stack (dtot, summed once per
    // period for the layer-dropping shortcut), then with the thickness of the oscillatory layers (a compare and an add per
    // layer); the sum of square roots itself is left to the few brackets that pass both (Love, ten layers: it cost 5 % of the
    // root search when every bracket formed it).
    float dtot = 0.0f;
    auto bracket_phase = [&](float c1, float c2, int mm) -> float {
        const float om = 6.2831853f * __builtin_amdgcn_rcpf(T);
        const float i1 = __builtin_amdgcn_rcpf(c1 * c1), i2 = __builtin_amdgcn_rcpf(c2 * c2);
        const float sq = 1.001f * om * sqrt_hw(fmaxf(i1 - i2, 0.0f));
        if (sq * dtot * ((KIND == 2) ? 2.0f : 1.0f) <= A.phimulti) return 0.0f;
        float dosc = 0.0f;
        for (int i = j; i < mm - 1; i += G) {
            const float d = W_D(i);
            if (KIND == 2) dosc += ((W_IB2(i) > i2) ? d : 0.0f) + ((W_IA2(i) > i2) ? d : 0.0f);
            else           dosc += (W_B(i) < c2) ? d : 0.0f;
        }
#pragma unroll
        for (int d = G >> 1; d > 0; d >>= 1) dosc += __shfl_xor(dosc, d);
        if (sq * dosc <= A.phimulti) return 0.0f;
        float sum = 0.0f;
        for (int i = j; i < mm - 1; i += G) {
            const float od = om * W_D(i);
            const float ib2 = (KIND == 2) ? W_IB2(i) : W_IR(i) * W_R(i);       // 1/b^2 (0: liquid)
            sum += od * (sqrt_hw(fmaxf(ib2 - i2, 0.0f)) - sqrt_hw(fmaxf(ib2 - i1, 0.0f)));
            if (KIND == 2) {
                const float ia2 = W_IA2(i);
                sum += od * (sqrt_hw(fmaxf(ia2 - i2, 0.0f)) - sqrt_hw(fmaxf(ia2 - i1, 0.0f)));
            }
        }
#pragma unroll
        for (int d = G >> 1; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        return fabsf(sum);
    };

    // Production kernel: can the reference's arithmetic overflow fp32 in this period although the production recursion stays
    // finite?  Rayleigh (DLTAR4 normalises per layer): a matrix ENTRY.  The largest entry is a51 ~ rhoc^2 g^4 rsinp rsinq <= rhoc^2 g^4 e^(pm+qm)
    // with pm + qm <= 2 k d.  Bound it per stack (thickest layer, largest rho and Vs: prep kernel) at the lowest
    // trial velocity of the period; beyond e^84 the stack goes to the exact fallback.
    // Love: DLTAR1 carries (ut, tt) through the layers WITHOUT normalisation (surfa.f:143-179): across evanescent layers the pair
    // grows like exp(sum of k d sqrt(1 - c^2/b^2)) and overflows fp32 beyond e^88 (or a layer's exp(q) underflows and its
    // reciprocal is inf) - the reference then scans NaNs and returns the edge of the overflowed region as the root, while the
    // production recursion stays finite and finds the true one.  Layer dropping bounds that sum: the layer at which the
    // evanescent thickness passes 4 c T becomes the half space, so the layers above it hold at most k x 4 c T = 8 pi of
    // exponent - EXCEPT when the TOP layer alone passes it (mmax is at least 2, surfa.f:105: the top layer stays a layer
    // whatever its thickness).  That one product, at the period's lowest trial velocity, decides: from e^76 on (the rest of the
    // margin: the 8 pi of further layers are not possible then, rho b^2 rb factors are) the stack goes to the exact fallback.
    // 200-km top layers at T < 3 s; no stack of the bench workloads.
    auto entry_overflow_risk = [&](float c_lo) -> bool {
        if (EXACT || !team_valid) return false;
        if (KIND == 1) {
            const float bb = W_B(0);                                        // (water on top, b = 0: never counted, never kept)
            if (!(bb > c_lo)) return !(c_lo > 0.0f && T > 0.0f);
            const float q0 = 6.2831853f * __builtin_amdgcn_rcpf(c_lo * T) * W_D(0) *
                             sqrt_hw(fmaxf(1.0f - c_lo * c_lo * __builtin_amdgcn_rcpf(bb * bb), 0.0f));
            return !(q0 < 76.0f);                                           // also when c_lo or T is not positive
        }
        const float hthick = A.ovf[b], lnrho2 = A.ovf[(size_t)B + b], lng4 = A.ovf[2 * (size_t)B + b];
        const float c_hi = W_B(mm_carry - 1) + 0.31f;                      // upper guard of the scan, calcul.f:166
        const float lnmag = 12.566371f * hthick / (c_lo * T) + lnrho2 + 4.0f * __logf(c_hi) +
                            fmaxf(lng4 - 8.0f * __logf(c_lo), 0.0f);
        return !(lnmag < 84.0f);                                           // also when c_lo or T is not positive
    };

    // Layer dropping (surfa.f:94-105) picks the first layer at which the thickness summed over the layers with
    // c < b exceeds 4 c T.  When the thickness of ALL n layers in the working stack (stale deep ones included) stays
    // below 4 c T at the period's lowest trial velocity, no trial of the period can drop anything: mmax = n without
    // walking the stack (three quarters of the bench workload's periods).  1e-5 covers the rounding of the partial sums.
    bool nodrop = false;
    auto no_drop_possible = [&](float c_lo) -> bool {
        float dsum = 0.0f;
        for (int i = j; i < n; i += G) dsum += W_D(i);
#pragma unroll
        for (int d = G >> 1; d > 0; d >>= 1) dsum += __shfl_xor(dsum, d);
        dtot = dsum;                                                       // (bracket_phase's first bound)
        return dsum * 1.00001f <= FACT * c_lo * T;
    };

    if (st != ST_DONE) {
        T = A.per[k];
        // clear the slot (a new process sees zeroed COMMON /d/)
        for (int i = j; i < Lcap; i += G) { W_IR(i) = 0.0f; W_B(i) = 0.0f; W_R(i) = 0.0f; W_D(i) = 0.0f; if (KIND == 2) { W_IA2(i) = 0.0f; W_IB2(i) = 0.0f; } }
        build(n);
        b1top = W_B(0);
        // first guess, fast_surf.f:157-171
        const bool water = M_AT(F_VS, 0) < 0.1f;
        const int il = water ? 1 : 0;
        const float b_corr = M_AT(F_QS, il) * logf(1.0f / T) / PI_REF;
        float qq = M_AT(F_VS, il);
        if (KIND == 2) qq = 0.9f * qq;
        p0c = qq * (1.0f + b_corr);
        if (water) p0c = 0.5f;
        first = true;
        nodrop = no_drop_possible(p0c);
        defer = (!EXACT && A.strict != 0) || entry_overflow_risk(p0c);    // SURFDISP_STRICT: everything to the exact kernel
        // CERT: a period in which no trial can drop layers (one eigenproblem for every trial velocity) starts on the coarse grid
        if (CERT) coarse = nodrop;
    }

    int wprio = -1;
    const bool LOCK = !EXACT && (INDEP ? A.lockstep >= 2 : A.lockstep != 0);
    // Pure scan passes (every team of the wavefront scans, waits for the refine pass or is done: nine passes in ten) take
    // a lean body after the evaluation - the crossing and guard tests, one permute per value instead of fifteen, and only
    // the bracket / carry bookkeeping of the scan branch below, with the same values and decisions.  Default scan of two-lane
    // teams only (the headline's pipelined launch: root search 1.39 -> 1.36 ms, profiles/r08a); teams of 4 .. 32 lanes
    // gained nothing measurable from it and the deep-stack c5 leg lost 1 % to the larger kernel, 64 lanes lost a wavefront per
    // SIMD (Love: six more VGPRs).
#ifdef SD_DEBUG_TRIALS
    constexpr bool LEAN = false;
#else
    constexpr bool LEAN = !FAST && !EXACT && !INDEP && (G == 2);
#endif
    // LEAN_BHS (the Rayleigh instantiation, the headline's root search): the lean body's upper guard compares the trial with
    // the half-space b the evaluation hands back - a register it held a few instructions earlier - instead of reading
    // W_B(mmj - 1), the same LDS word, again: that read, its address and its wait stood alone between the evaluation and
    // the team's decision.  Root search of one bench batch with two-lane teams 1.848 -> 1.809 ms (-2.1 %, spread 7 us); the
    // three-batch headline gains 1-2 %, which is close to its run-to-run spread (profiles/r11a, where the moves that gained
    // nothing or lost are recorded too).  -DSD_NO_GUARD_HANDBACK builds the parent's code for the A/B.
#ifdef SD_NO_GUARD_HANDBACK
    constexpr bool LEAN_BHS = false;
#else
    constexpr bool LEAN_BHS = LEAN && (KIND == 2);
#endif
    // LEAN2 (the same instantiation, lock step): a lean pass evaluates TWO grid points per lane, one after the other through
    // the one copy of the evaluation - A, the point of a single pass, then B two grid steps further up - and the team
    // decides once over its four points in grid order (lane 0 A, lane 1 A, lane 0 B, lane 1 B: scan_decide4,
    // surfdisp_k_scan.h), with the outcome of two consecutive lean passes: the priority test, the state tests, the trial
    // choice's selects and the bracket / carry bookkeeping are paid once per four grid points instead of once per two.
    // Between the evaluations only A's events are formed (wavefront masks in scalar registers; a lane keeps A's value and
    // mm): a team with a crossing, the guard, a non-finite value or a pending deferral at A sits B out as a waiting team
    // does, and when no team is left to scan on, B is not run at all - the wavefront evaluates exactly the rounds it did.
    // Without lock step a bracket starts refining in the very next pass: those launches take the general body.
#ifdef SD_NO_DOUBLE_SCAN
    constexpr bool LEAN2 = false;
#else
    constexpr bool LEAN2 = LEAN_BHS;
#endif
    // NEVILL's prologue, surfa.f:12-16, from the scan's bracket (del1 is the scan's value, whatever layer dropping it was computed
    // with - as in the reference)
    auto nevill_start = [&]() {
        nv_ic = 0; nv_nev = 1; nv_m = 1;
        croot = (p0c + cb) / 2.0f;                             // c3, evaluated by the next pass
        st = (KIND == 1 && !EXACT) ? ST_NEVILL0 : ST_NEVILL;   // (Love: first the end values in the reference's arithmetic)
        sub = 0;
        if (!EXACT && j == 0 && A.amb_count) atomicAdd(A.amb_count, 1);     // (statistics)
    };
    while (__any(st != ST_DONE)) {
#ifdef SD_WAVECLOCK
        const unsigned long long wp0 = __builtin_readcyclecounter();
#endif
        // The SIMD arbitrates between its wavefronts by priority, then age: left alone, the four wavefronts of a
        // SIMD finish one after the other and the last one runs alone for a seventh of the kernel.  Let a wavefront
        // that is behind (period index of its first team) go first: 2.39 -> 2.15 ms for one bench batch (profiles/r02c).
        // Not for narrow teams (< 8 lanes) when the caller keeps a second batch in flight (SURFDISP_PIPELINED): there the age
        // order lets the older batch drain while the younger one fills the machine (three bench batches in flight: 38.4 M
        // solves/s without, 37.7 M with).  Wide teams keep it also then: the two root searches of a joint Rayleigh + Love
        // solve of 64-layer stacks, 5.59 -> 5.23 ms (r03).  SURFDISP_BALANCE=0 / 1 forces it.
        if (!INDEP && A.balance) {
            const int kw = __builtin_amdgcn_readfirstlane(k);
            const int pr = 3 - min(3, (4 * kw) / max(P, 1));
            if (pr != wprio) {
                wprio = pr;
                if (pr == 3) __builtin_amdgcn_s_setprio(3);
                else if (pr == 2) __builtin_amdgcn_s_setprio(2);
                else if (pr == 1) __builtin_amdgcn_s_setprio(1);
                else __builtin_amdgcn_s_setprio(0);
            }
        }
        const bool lean = LEAN && A.scan_general == 0 && (!LEAN2 || LOCK) && __all(st == ST_SCAN || st == ST_WREF || st == ST_DONE);
        // ---------------------------------------------------------------- choose the trial point
        float cj = 1.0f;
        int mmj = 2, start = 1;
        bool eval = (st != ST_DONE) && (st != ST_WREF) && (st != ST_WEND);
        const int js = (OVERLAP && ell_pend && st == ST_SCAN) ? j - 2 : j;   // scan-lane index in the team
        if (st == ST_SCAN) {
            // exact fp32 grid of the reference: c2 = c1 + dc repeatedly (calcul.f:157,161)
            const int nadd = (CERT && coarse) ? FSTRIDE * (first ? js : js + 1) : (first ? js : js + 1);   // (CERT may start a period on the coarse grid)
            cj = p0c;
            if (CERT) {
#pragma unroll
                for (int i = 0; i < FSTRIDE * G; ++i) if (i < nadd) cj = cj + DC;
            } else {
#pragma unroll
                for (int i = 0; i < G; ++i) if (i < nadd) cj = cj + DC;
            }
            mmj = nodrop ? (n < 2 ? 2 : n) : drop_layers(wq, LS, S, n, cj, T);   // idrop=0 before every scan trial
        } else if (st == ST_NEVILL0) {
            // the scan's two end values again (del1 with the layer dropping of ITS trial, del2's is the frozen one)
            const bool hi = (G == 1) ? (sub != 0) : ((j & 1) != 0);
            cj = hi ? cb : p0c; mmj = hi ? mm_frozen : p0mm;
        } else if (st == ST_NEVILL) {
            cj = croot; mmj = mm_frozen;                       // NEVILL's c3, idrop = 1
        } else if (st == ST_REFINE) {
            const float w = cb - p0c;
            cj = p0c + (float)(j + 1) * (w * (1.0f / (float)(G + 1)));
            if (G <= 4 && G > 1 && p0ok && w > 16.0f * CLUSTER_DC) {
                // small teams: instead of G equidistant points, cluster them around the secant
                // estimate (spacing CLUSTER_DC).  Delta(c) is smooth across a 0.01 bracket, so the
                // root normally falls between two neighbours and the next acceptance test passes
                // (one refine pass instead of two); if it does not, the sign pattern still shrinks
                // the bracket and the next pass clusters around a better estimate.
                // (estimates of where to put trial points and of the root inside a bracket <= 0.01 km/s wide: v_rcp_f32
                // quotients, 1 ulp - an IEEE division is ten instructions, and a dozen of them sat on every pass)
                float ts = -p0d * w * __builtin_amdgcn_rcpf(db - p0d);
                // offsets in units of CLUSTER_DC: tight around the estimate, wider outside, so that a
                // poorer estimate still lands between two points
                const float off = (G == 4) ? ((j == 0) ? -4.0f : (j == 1) ? -1.0f : (j == 2) ? 1.0f : 4.0f)
                                           : ((j == 0) ? -1.5f : 1.5f);
                const float half = ((G == 4) ? 4.0f : 1.5f) * CLUSTER_DC;
                ts = fminf(fmaxf(ts, half + CLUSTER_DC), w - half - CLUSTER_DC);
                if (ts == ts) cj = p0c + (ts + off * CLUSTER_DC);
            }
            mmj = mm_frozen;                                   // frozen as NEVILL sees it
        } else if (st == ST_ELLIP) {
            cj = croot; mmj = mm_frozen;
            start = (G == 1) ? 2 + sub : 2 + j;
            eval = (G == 1) || (j < 2);
        }
        float val = 0.0f, phj = 0.0f;
        int kcj = 0; bool kuncj = false;                       // Sturm count of this lane's trial (CERT)
#ifdef SD_WAVECLOCK
        unsigned long long we0 = __builtin_readcyclecounter();
        wcyc_pre += we0 - wp0;                                 // priority, trial velocities, layer dropping
        ++wpasses;
        auto wcount = [&]() {                                  // (once per evaluation round: LEAN2 runs two in a pass)
            const unsigned long long lead = __ballot(j == 0);
            wn_scan += __popcll(__ballot(st == ST_SCAN) & lead); wn_refine += __popcll(__ballot(st == ST_REFINE) & lead);
            wn_nevill += __popcll(__ballot(st == ST_NEVILL) & lead); wn_ellip += __popcll(__ballot(st == ST_ELLIP) & lead);
            wn_idle += __popcll(__ballot(st == ST_DONE || st == ST_WREF || st == ST_WEND) & lead);
            int mx = eval ? mmj : 0, sm = eval ? mmj : 0;
            for (int d = 32; d > 0; d >>= 1) { mx = max(mx, __shfl_xor(mx, d)); sm += __shfl_xor(sm, d); }
            wtrip += mx; wlanelayers += sm; wlanes += __popcll(__ballot(eval));
        };
        wcount();
#endif
        float vmag = 0.0f;                                     // magnitude of the terms the value is the sum of (production recursion)
        [[maybe_unused]] float bhsj = 0.0f;                    // b of this lane's effective half space (LEAN_BHS)
        // LEAN2: what a lane keeps of its point A while it evaluates point B - the value and mm in two registers, the raw guard
        // test as a lane mask - and "second": this pass ran both rounds
        [[maybe_unused]] float a_val = 0.0f;
        [[maybe_unused]] int a_mm = 0;
        [[maybe_unused]] bool a_g = false, second = false;
        // (one code instance of the evaluation for both points: the loop stays rolled, so A and B run the same instructions)
#pragma nounroll
        for (;;) {
        if (eval) {
            const bool want_mag = want_ratio && st == ST_ELLIP;   // (the in-kernel ellipticity passes' cancellation test)
            if (KIND == 2) val = EXACT ? delta_rayleigh_ref(wq, LS, S, mmj, cj, T, start)
                                       : delta_rayleigh<(G != 2) && !FAST, CERT, (G <= 16)>(wq, LS, S, mmj, cj, T, start, phj, &vmag, want_mag, &kcj, &kuncj, coarse,
                                                                                                            LEAN_BHS ? &bhsj : nullptr
#ifdef SD_WAVECLOCK
                                                                                                            , wsec
#endif
                                                                                                            );
            // Love, NEVILL passes of the production kernel: DLTAR1 statement by statement on the production working stack (it holds
            // b, rho, d as the exact kernel's does).  A bracket goes to NEVILL because it may hold several roots, and which of them
            // NEVILL lands on depends on the VALUES it sees (its 10 x rule, its interpolation) - with e^{kd} of hundreds of km of
            // layer the production recursion's values differ from the reference's by whole orders of magnitude, or are inf where
            // those are finite (r04 soak, thick-layer family, Love: 2e-4 of the stacks on another overtone with the production
            // values, 1.4e-2 before there was a NEVILL for such brackets at all).
            else if (!EXACT && (st == ST_NEVILL || st == ST_NEVILL0)) val = delta_love_ref_body(wq, LS, S, mmj, cj, T);
            else           val = EXACT ? delta_love_ref(wq, LS, S, mmj, cj, T)
                                       : delta_love<CERT, (G <= 16)>(wq, LS, S, mmj, cj, T, phj, kcj, kuncj, coarse);   // counts only where they are compared: coarse passes
        }
        if constexpr (LEAN2) {
            if (lean && !second) {
                // point A's events.  The teams that scan on: no crossing, no guard, every value finite, no deferral pending
                // (entry_overflow_risk at the period's start, acted on at the end of its first pass)
                const bool scan = (st == ST_SCAN);
                const float od = pair_swap(val);
                bool cr;
                const bool g = (cj < 0.8f * b1top) || !(cj < bhsj + 0.3f);             // calcul.f:165-166
                const bool ev = scan_event((j == 0) ? p0d : od, !(first && j == 0), val, g, &cr);
                const int hit = (int)(scan && (ev || defer || !fin(val)));
                const bool go = scan && ((hit | pair_swap(hit)) == 0);                 // (neither lane of the team)
                if (__any(go)) {
#ifdef SD_WAVECLOCK
                    const unsigned long long wa0 = __builtin_readcyclecounter();
                    wcyc_eval += wa0 - we0;
#endif
                    second = true;
                    a_val = val; a_mm = mmj; a_g = g;
                    eval = go;
                    cj = cj + DC; cj = cj + DC;                // the grid of the next single pass: its p0c is lane 1's A
                    mmj = nodrop ? (n < 2 ? 2 : n) : drop_layers(wq, LS, S, n, cj, T);
                    val = 0.0f;
#ifdef SD_WAVECLOCK
                    we0 = __builtin_readcyclecounter();
                    wcyc_pre += we0 - wa0; ++wn_double;
                    wcount();
#endif
                    continue;
                }
            }
        }
        break;
        }
        // The in-kernel ellipticity passes (two-lane teams): a closure that is the remainder of a cancellation - |value| below
        // A.ell_ambig of the terms it is the sum of - marks the (stack, period) for the ellipticity kernel, which evaluates both
        // passes with the reference's arithmetic on the replayed working stack (see there)
        const bool ell_amb = !EXACT && want_ratio && eval && st == ST_ELLIP && A.ell_ambig != 0.0f &&
                             (A.ell_ambig < 0.0f || fabsf(val) < A.ell_ambig * vmag ||
                              cj * cj < ell_c2min);                                       // see surfdisp_ellip_kernel
#ifdef SD_WAVECLOCK
        const unsigned long long wl0 = __builtin_readcyclecounter();
        wcyc_eval += wl0 - we0;
#endif
        if constexpr (LEAN2) if (lean) {
            // ------------------------------------------------------------ lean scan pass of one or two rounds (see LEAN2)
            // Every lane of a team gathers the team's points in grid order - values and mm from the other lane by DPP, the
            // trial velocities by the grid's own additions from p0c - and takes the same decision.
            const bool scan = (st == ST_SCAN);
            const bool j0 = (j == 0);
            const ScanPt p0 = {p0d, p0c, p0mm, false};
            const float c0 = first ? p0c : p0c + DC, c1 = c0 + DC;
            const float av = second ? a_val : val;
            const int am = second ? a_mm : mmj;
            const bool ag = second ? a_g : ((cj < 0.8f * b1top) || !(cj < bhsj + 0.3f));
            const float oav = pair_swap(av);
            const int oam = pair_swap(am);
            const bool oag = pair_swap((int)ag) != 0;
            ScanOut o;
            bool allfin;
            if (second) {
                const float c2 = c1 + DC, c3 = c2 + DC;
                const bool bg = (cj < 0.8f * b1top) || !(cj < bhsj + 0.3f);
                const float obv = pair_swap(val);
                const int obm = pair_swap(mmj);
                const bool obg = pair_swap((int)bg) != 0;
                const ScanPt pt[4] = {{j0 ? av : oav, c0, j0 ? am : oam, j0 ? ag : oag}, {j0 ? oav : av, c1, j0 ? oam : am, j0 ? oag : ag},
                                      {j0 ? val : obv, c2, j0 ? mmj : obm, j0 ? bg : obg}, {j0 ? obv : val, c3, j0 ? obm : mmj, j0 ? obg : bg}};
                o = scan_decide4(p0, first, pt);
                allfin = fin(av) && fin(oav) && fin(val) && fin(obv);   // (a team with its event at A has not evaluated B: 0)
            } else {
                const ScanPt pt[2] = {{j0 ? av : oav, c0, j0 ? am : oam, j0 ? ag : oag}, {j0 ? oav : av, c1, j0 ? oam : am, j0 ? oag : ag}};
                o = scan_decide2(p0, first, pt);
                allfin = fin(av) && fin(oav);
            }
            if (scan && !allfin) defer = true;                 // -> exact fallback kernel
            bool failed = false;
            if (scan) {
                if (o.e >= 0 && o.cross) {                     // bracket found -> refine (see the general body)
                    p0c = o.lo.c; p0d = o.lo.v; cb = o.hi.c; db = o.hi.v; mm_frozen = o.hi.mm; p0mm = o.lo.mm;
                    p0ok = (o.lo.mm == o.hi.mm);
                    if (o.e >= 2) first = false;
                    passes = 0;
                    st = ST_WREF;                              // (LOCK: see lean)
                } else if (o.e >= 0) {
                    failed = true;                             // label 250
                } else {
                    p0c = o.lo.c; p0d = o.lo.v; p0mm = o.lo.mm; first = false;
                    passes += second ? 2 : 1;
                    if (passes > 100000) failed = true;
                }
            }
            if (defer) {
                if (j == 0) A.fb_list[atomicAdd(A.fb_count, 1)] = (int)tg;
                defer = false; st = ST_DONE; failed = false;
            }
            if (failed) {
                status = (k == 0) ? SURFDISP_NOROOT : SURFDISP_PARTIAL;
                st = ST_DONE;
            }
            if (!__any(st == ST_SCAN) && st == ST_WREF) {      // (no team ends its period in a scan pass)
                st = ST_REFINE;
                if (bracket_phase(p0c, cb, mm_frozen) > A.phimulti) nevill_start();
            }
#ifdef SD_WAVECLOCK
            wcyc_lean += __builtin_readcyclecounter() - wl0; ++wn_lean;
#endif
            continue;
        }
        if (!LEAN2 && lean) {
            // ------------------------------------------------------------ lean scan pass (see LEAN)
            // What the general body below does for ST_SCAN, ST_WREF and ST_DONE teams, and nothing else.  Per team, the lane q
            // whose trial is kept: the first one with a crossing or the guard (bracket: q and the trial before it), else the
            // last one (the carry).  Teams of two read the other lane with DPP; q and the trial before it are then both in
            // hand.  (Other team sizes, if enabled above: they permute from lane - 1 and from q.)
            const bool scan = (st == ST_SCAN);
            auto negnan = [](float x) { return signbit(x) && !(x != x); };   // (as below)
            float oc = cj, od = val; int omm = mmj;            // G == 2: the other lane of the team
            float sc = p0c, sv_ = p0d; int smm = p0mm;         // the previous lane's trial
            if (G == 2) {
                oc = pair_swap(cj); od = pair_swap(val); omm = pair_swap(mmj);
                sc = oc; sv_ = od; smm = omm;
            } else if (G > 2) {
                const int lm1 = (lane + 63) & 63;
                sc = __shfl(cj, lm1); sv_ = __shfl(val, lm1); smm = __shfl(mmj, lm1);
            }
            const float pc = (j == 0) ? p0c : sc, pd = (j == 0) ? p0d : sv_;
            const int pmm = (j == 0) ? p0mm : smm;
            const bool has_prev = !(first && j == 0);
            const bool cross = has_prev && (negnan(val) != negnan(pd));
            bool guard = false;
            if (scan && has_prev && !cross) {                  // calcul.f:165-166
                if constexpr (LEAN_BHS) guard = (cj < 0.8f * b1top) || !(cj < bhsj + 0.3f);
                else                    guard = (cj < 0.8f * b1top) || !(cj < W_B(mmj - 1) + 0.3f);
            }
            const unsigned long long em = __ballot(scan && (cross || guard)) & tmask;
            const int fl = em ? (__ffsll((long long)em) - 1) : -1;
            const int q = (fl < 0) ? tbase + G - 1 : fl;
            const bool q_cross = ((__ballot(cross) >> q) & 1ull) != 0ull;
            float q_c, q_d, q_pc, q_pd;
            int q_mm, q_pmm;
            if (G == 1) {
                q_c = cj; q_d = val; q_mm = mmj; q_pc = pc; q_pd = pd; q_pmm = pmm;
            } else if (G == 2) {
                const bool mine = (q == lane), q_lo = (q == tbase);
                q_c = mine ? cj : oc; q_d = mine ? val : od; q_mm = mine ? mmj : omm;
                q_pc = q_lo ? p0c : ((j == 0) ? cj : oc);     // before the team's second lane: its first
                q_pd = q_lo ? p0d : ((j == 0) ? val : od);
                q_pmm = q_lo ? p0mm : ((j == 0) ? mmj : omm);
            } else {
                q_c = __shfl(cj, q); q_d = __shfl(val, q); q_mm = __shfl(mmj, q);
                q_pc = __shfl(pc, q); q_pd = __shfl(pd, q); q_pmm = __shfl(pmm, q);
            }
            if (scan && ((__ballot(scan && !fin(val)) & tmask) != 0ull)) defer = true;   // -> exact fallback kernel
            bool failed = false;
            if (scan) {
                ++passes;
                if (fl >= 0 && q_cross) {                      // bracket found -> refine (see the general body)
                    p0c = q_pc; p0d = q_pd; cb = q_c; db = q_d; mm_frozen = q_mm; p0mm = q_pmm;
                    p0ok = (q_pmm == q_mm);
                    passes = 0;
                    st = LOCK ? ST_WREF : ST_REFINE;
                    if (!LOCK && bracket_phase(p0c, cb, mm_frozen) > A.phimulti) nevill_start();
                } else if (fl >= 0) {
                    failed = true;                             // label 250
                } else {
                    p0c = q_c; p0d = q_d; p0mm = q_mm; first = false;
                    if (passes > 100000) failed = true;
                }
            }
            if (defer) {
                if (j == 0) A.fb_list[atomicAdd(A.fb_count, 1)] = (int)tg;
                defer = false; st = ST_DONE; failed = false;
            }
            if (failed) {
                status = (k == 0) ? SURFDISP_NOROOT : SURFDISP_PARTIAL;
                st = ST_DONE;
            }
            if (LOCK && !__any(st == ST_SCAN) && st == ST_WREF) {   // (no team ends its period in a scan pass)
                st = ST_REFINE;
                if (bracket_phase(p0c, cb, mm_frozen) > A.phimulti) nevill_start();
            }
#ifdef SD_WAVECLOCK
            wcyc_lean += __builtin_readcyclecounter() - wl0; ++wn_lean;
#endif
            continue;
        }
        // ---------------------------------------------------------------- team-level decisions
        const int lm1 = (lane + 63) & 63;
        const float sc = __shfl(cj, lm1), sv_ = __shfl(val, lm1);
        const float pc = (j == 0) ? p0c : sc;
        const float pd = (j == 0) ? p0d : sv_;
        const int smm = __shfl(mmj, lm1);
        const int pmm = (j == 0) ? p0mm : smm;
        const int kpk = CERT ? ((kcj + 4096) | (kuncj ? 0x40000000 : 0)) : 0;          // count | unsafe flag, packed
        const int sKp = CERT ? __shfl(kpk, lm1) : 0;                                   // ... of the previous lane
        const int pKp = (j == 0) ? p0Kp : sKp;
        const bool searching = ((st == ST_SCAN) || (st == ST_REFINE)) ;
        const bool has_prev = !((st == ST_SCAN) && first && (js == 0));
        auto negnan = [](float x) { return signbit(x) && !(x != x); };   // a NaN compares as positive, see below
        const bool cross = has_prev && (negnan(val) != negnan(pd));
#ifdef SD_DEBUG_TRIALS   // (developer build: every evaluated trial of a one-stack call)
        if (A.B == 1 && eval && k == SD_DEBUG_TRIALS && cj > SD_DEBUG_CMIN)
            printf("k %d pass %d st %d lane %d c %.7f val % .6e mm %d count %d unsafe %d coarse %d | p0c %.7f p0d % .4e cb %.7f db % .4e\n", k, passes, st, j, cj, val, mmj, kcj, (int)kuncj, (int)coarse, p0c, p0d, cb, db);
#endif
        bool guard = false;
        if (st == ST_SCAN && has_prev && !cross)               // calcul.f:165-166
            guard = (cj < 0.8f * b1top) || !(cj < W_B(mmj - 1) + 0.3f);
        // coarse pass: the interval (previous coarse point, this one) may be skipped only if both ends were evaluated with the
        // same effective half space and carry equal, safe mode counts.  Anything else is rescanned point by point.
        bool uncert = false, back0 = false;
        if (CERT) {
            if (coarse && st == ST_SCAN) {
                // below the half-space velocity by two coarse steps (there the problem stops being an eigenvalue problem)
                const bool near_hs = !(cj < W_B(mmj - 1) - 2.0f * (float)FSTRIDE * DC);
                // ... and the scan's lower guard (calcul.f:165: a trial below 0.8 b(1) ends the search) looks at every grid
                // point: the first one a skip would pass over is pc + dc
                const bool low_guard = (pc + DC) < 0.8f * b1top;
                uncert = has_prev && (near_hs || low_guard || !((pmm == mmj) && fin(pd) && fin(val) && !kuncj && (pKp == kpk)));
            }
        }
        const bool ev = searching && (cross || guard || uncert);
        const unsigned long long em = __ballot(ev) & tmask;
        const int fl = em ? (__ffsll((long long)em) - 1) : -1;
        const int src = (fl < 0) ? tbase : fl;
        const float e_c = __shfl(cj, src), e_d = __shfl(val, src);
        const float e_pc = __shfl(pc, src), e_pd = __shfl(pd, src);
        const int e_mm = __shfl(mmj, src);
        const int e_pmm = __shfl(pmm, src);
        const int l_mm = __shfl(mmj, tbase + G - 1);
        const int e_cross = __shfl((int)cross, src);
        const int t_back0 = CERT ? __shfl((int)back0, tbase) : 0;
        const int lastl = tbase + G - 1;
        const float l_c = __shfl(cj, lastl), l_d = __shfl(val, lastl);
        const float l_phi = CERT ? __shfl(phj, lastl) : 0.0f;
        const int l_Kp = CERT ? __shfl(kpk, lastl) : 0;
        const int e_pKp = CERT ? __shfl(pKp, src) : 0;
        // the values of the team's first two lanes: the two ellipticity recursions, and NEVILL's del3 (every lane of the team
        // evaluated the same c3) - only where some team of the wavefront needs them (not in a scan or refine pass of a c+U call)
        float v0 = 0.0f, v1 = 0.0f;
        if (__any((st == ST_ELLIP) | (st == ST_NEVILL) | (st == ST_NEVILL0))) { v0 = __shfl(val, tbase); v1 = __shfl(val, (G > 1) ? tbase + 1 : tbase); }
        // what only a REFINE pass reads (wavefront-uniform test: in lock step most passes have no refining team):
        // the right neighbour of the crossing lane, the lane before the last one, and - the fourth point of the second
        // three-point estimate - two lanes below / above the crossing lane and two before the last one
        float e_nc = 0.0f, e_nd = 0.0f, pl_c = 0.0f, pl_d = 0.0f, e_ppc = 0.0f, e_ppd = 0.0f, e_n2c = 0.0f, e_n2d = 0.0f,
              pl2_c = 0.0f, pl2_d = 0.0f;
        int pl_mm = 0;
        if (CERT || __any(st == ST_REFINE)) {
            const int nxt = (src < lastl) ? src + 1 : lastl;
            e_nc = __shfl(cj, nxt); e_nd = __shfl(val, nxt);
            const int pl = (G > 1) ? lastl - 1 : lastl;
            pl_c = __shfl(cj, pl); pl_d = __shfl(val, pl);
            if (CERT) pl_mm = __shfl(mmj, pl);
            const int lm2s = (src - 2 >= tbase) ? src - 2 : tbase;
            e_ppc = __shfl(cj, lm2s); e_ppd = __shfl(val, lm2s);
            const int nx2 = (src + 2 <= lastl) ? src + 2 : lastl;
            e_n2c = __shfl(cj, nx2); e_n2d = __shfl(val, nx2);
            const int pl2 = (G > 2) ? lastl - 2 : lastl;
            pl2_c = __shfl(cj, pl2); pl2_d = __shfl(val, pl2);
        }
        const bool had_ell = OVERLAP && ell_pend && (st == ST_SCAN);

        bool solved = false, failed = false;
        // A secular function that left the fp32 range (NaN / inf: products of e^{k d} terms beyond 3e38 in very
        // thick layers at short periods).  The reference's scan compares SIGN(1., del): the NaNs its arithmetic
        // produces carry the sign bit (x86 default NaN) and both secular functions return the NEGATED recursion
        // result (surfa.f:179,357), so a NaN passes as a positive value (negnan above).  In NEVILL a NaN end value
        // makes the Neville step return a NaN abscissa, and the arithmetic IFs of surfa.f:32-34 send a NaN to their
        // third label, i.e. to a BISECTION step (flang and gfortran lower `if (x) l1,l2,l3` to x<0, x==0, else):
        // the reference keeps halving on signs alone and returns the edge of the overflowed region as that
        // period's root (pinned bit for bit by the fixtures tests/golden/ref_families.npz).  Same here: the
        // subdivision below decides on signs with NaN = positive, and interpolation is only trusted on finite
        // values (a non-finite estimate falls back to the bracket's low end once it is 1e-6 wide).
        // What NEVILL cannot do is separate two fp32 numbers above 16 km/s (spacing 1.9e-6 > its 1e-6 tolerance,
        // surfa.f:10,44): its 50-cycle limit trips (surfa.f:17-27), calcul.f:172-189 jumps to 9999 and the whole
        // call returns nothing, also the periods already solved - SURFDISP_NUMERIC (see `fatal` in REFINE below).
        bool fatal = false, multi = false;
        if (!EXACT) {
            // what this kernel does not reproduce faithfully (see the template flags)
            const bool nonfin = ((__ballot(eval && !fin(val)) & tmask) != 0ull);
            if (st != ST_DONE && nonfin) defer = true;         // -> exact fallback kernel
            if (st == ST_REFINE && passes == 0) {              // first refine pass: sign changes across the bracket
                const int ncross = __popcll(__ballot(searching && cross) & tmask) + ((negnan(l_d) != negnan(db)) ? 1 : 0);
                multi = ncross >= 2;                           // -> NEVILL for this period
            }
        }
        if (CERT && st == ST_SCAN && coarse) {
            ++passes;
            if (fl >= 0) {                                     // rescan this interval point by point
                p0c = e_pc; p0d = e_pd; p0mm = e_pmm;
                if (CERT) p0Kp = e_pKp;
                const bool e_back = (fl == tbase) && (t_back0 != 0);
                if (e_back) { p0c = q0c; p0d = q0d; p0mm = q0mm; }
                // after a failed certificate stay on the fine grid for the next interval too (a restart at q0
                // has two intervals to cover; a change of the layer dropping usually sits close to the root)
                coarse = false; fine_left = (e_cross && !e_back) ? FSTRIDE : 2 * FSTRIDE; q0ok = false;
                if (CERT) { fine_left = FSTRIDE; first = false; }      // (the certified scan rescans the one interval)
            } else {
                q0c = pl_c; q0d = pl_d; q0mm = pl_mm; q0ok = true;
                p0c = l_c; p0d = l_d; p0mm = l_mm; p0phi = l_phi;
                if (CERT) { p0Kp = l_Kp; first = false; }
            }
        } else if (st == ST_SCAN) {
            ++passes;
            if (fl >= 0 && e_cross) {                          // bracket found -> refine
                p0c = e_pc; p0d = e_pd; cb = e_c; db = e_d; mm_frozen = e_mm; p0mm = e_pmm;
                // the low end was evaluated with ITS OWN layer dropping (idrop=0 per scan trial); if
                // that differs from the frozen one its magnitude belongs to a different function
                // and only its sign may be used (NEVILL's 10x guard, surfa.f:47-51, covers this)
                p0ok = (e_pmm == e_mm);
                passes = 0;
                st = LOCK ? ST_WREF : ST_REFINE;
                // EXACT: always NEVILL.  Production: NEVILL (statement by statement, from the scan's bracket) when the
                // bracket may hold SEVERAL roots: consecutive modes are ~pi apart in the vertical phase (sum of omega d
                // sqrt(1/v^2 - 1/c^2) over the oscillatory layers), so a bracket across which it grows by more than A.phimulti
                // (1 rad; an ordinary bracket's growth is 1e-2) - thick soft layers at short periods, overtones 1e-3 km/s
                // apart - may hold more than one, which of them NEVILL lands on depends on its evaluation sequence, and a
                // team of a few lanes cannot see them: the subdivision's own test (`multi`: more than one sign change among
                // the G points of the first refine pass) only sees roots further apart than its points.  r04 soak: 4e-3 of
                // the soft-sediment family's Love stacks came back on another overtone (1 .. 15 % off) from teams of <= 8
                // lanes.  The phase is summed by the team, once per bracket (a layer per lane and turn).
                // (Lock step: the teams of a wavefront find their brackets in different passes, and a block run for one team
                // costs the wavefront as much as for all - the phase is summed when all of them leave ST_WREF together, below.)
                if (EXACT || (!LOCK && bracket_phase(p0c, cb, mm_frozen) > A.phimulti)) nevill_start();
            } else if (fl >= 0) {
                failed = true;                                 // label 250
            } else {
                p0c = l_c; p0d = l_d; p0mm = l_mm; first = false;
                if (CERT) p0Kp = l_Kp;
                if (CERT) { p0phi = l_phi; q0d = pl_d; q0mm = pl_mm; }    // pl: the fine point p0 - dc
                if (passes > 100000) failed = true;            // cannot happen: c grows by dc/pass
                if (CERT) {
                    fine_left -= had_ell ? G - 2 : G;
                    if (fine_left <= 0 && nodrop) { coarse = true; q0ok = false; }
                    // (CERT: fine passes carry no counts, so the coarse pass starts AT p0 - its first lane evaluates it again)
                    if (CERT && coarse) first = true;
                }
            }
        } else if (!EXACT && st == ST_REFINE && multi) {
            // more than one sign change inside the bracket: hand this period to NEVILL, from the scan's bracket
            // (p0c, cb and their values are still the scan's: this is the first refine pass).  (Sending the whole stack
            // to the exact fallback kernel instead changes nothing measurable: soak mismatch rates 1.70e-5 / 1.39e-5 ->
            // 1.71e-5 / 1.36e-5, profiles/r03a/ab_multi_defer.txt.)
            nv_ic = 0; nv_nev = 1; nv_m = 1;
            croot = (p0c + cb) / 2.0f;
            st = (KIND == 1) ? ST_NEVILL0 : ST_NEVILL;
            sub = 0;
        } else if (st == ST_NEVILL0) {
            if (G == 1) { if (sub == 0) { p0d = val; sub = 1; } else { db = val; st = ST_NEVILL; } }
            else { p0d = v0; db = v1; st = ST_NEVILL; }
        } else if (st == ST_NEVILL) {
            // NEVILL, statement by statement (surfa.f:17-83).  One evaluation per pass: del3 = Delta(c3) has just
            // been computed by every lane of the team (v0); what follows runs up to the next evaluation.
            // SIGN(1., x): the reference's NaNs are positive when they come out of the secular function (negnan
            // above) or are passed on by a subtraction, negative when a subtraction creates them (inf - inf: the
            // x86 default NaN).  No fused multiply-adds: the reference is built without contraction.
#pragma clang fp contract(off)
            auto sg = [](float x) { return (signbit(x) && !(x != x)) ? -1.0f : 1.0f; };
            auto sgsub = [&](float a, float bq) {
                const float r = a - bq;
                if (r != r) return ((a != a) || (bq != bq)) ? 1.0f : -1.0f;
                return signbit(r) ? -1.0f : 1.0f;
            };
            float c1 = p0c, c2 = cb, d1 = p0d, d2 = db, c3 = croot;
            const float d3 = v0;
            nv_ic = nv_ic + 1;
            bool fin_ = false;
            if (!(nv_ic < 50)) fatal = true;                   // TOO MANY CYCLES: lstop, calcul.f:172-189 -> 9999
            else {
                bool bis;
                if (c1 - c3 <= 0.0f) bis = (c2 - c3 <= 0.0f);  // 777 / 1320 / 1330: arithmetic IFs, a NaN
                else bis = !(c2 - c3 < 0.0f);                  // expression takes the third label
                if (!bis) {
                    const float s13s = sgsub(d1, d3), s32s = sgsub(d3, d2);            // label 1000
                    if (sg(d3) * sg(d1) <= 0.0f) { c2 = c3; d2 = d3; } else { c1 = c3; d1 = d3; }
                    if (fabsf(c1 - c2) - 0.1e-5f <= 0.0f) fin_ = true;                 // 1444: accur1
                    else {
                        if (s13s != s32s) nv_nev = 0;
                        const float ss1 = fabsf(d1), s1 = 0.1f * ss1, ss2 = fabsf(d2), s2 = 0.1f * ss2;
                        if (s1 > ss2 || s2 > ss1) bis = true;
                        else if (nv_nev == 0) bis = true;
                        else {
                            int m = nv_m;
                            if (nv_nev == 2) { nvx[m + 1] = c3; nvy[m + 1] = d3; }     // 1350
                            else { nvx[1] = c1; nvy[1] = d1; nvx[2] = c2; nvy[2] = d2; m = 1; }
                            const float ym1 = nvy[m + 1];
                            for (int kk = 1; kk <= m; ++kk) {                           // 1355-1360
                                const int jn = m - kk + 1;
                                const float yj = nvy[jn];
                                if (fabsf(ym1 - yj) <= 0.1e-7f) { bis = true; break; }
                                nvx[jn] = (-yj * nvx[jn + 1] + ym1 * nvx[jn]) / (ym1 - yj);
                            }
                            if (!bis) { c3 = nvx[1]; nv_nev = 2; nv_m = (m + 1 > 10) ? 10 : m + 1; }   // 21
                        }
                    }
                }
                if (!fin_ && bis) { c3 = (c1 + c2) / 2.0f; nv_nev = 1; nv_m = 1; }      // 1344
                p0c = c1; p0d = d1; cb = c2; db = d2; croot = c3;
            }
            if (fin_) {                                        // label 20: cc = c3
                if (croot <= W_B(mm_frozen - 1)) {             // calcul.f:191
                    if (want_ratio) { st = ST_ELLIP; sub = 0; } else solved = true;
                } else failed = true;
            }
        } else if (st == ST_REFINE) {
            // new bracket + one more known point next to it (for the final 3-point step)
            float tc, td;
            bool tok = true;
            float uc = 0.0f, ud = 0.0f;                        // a fourth point, on the other side where there is one
            bool uok = false;
            const float oa = p0c, oda = p0d, ob = cb, odb = db;
            const bool oaok = p0ok;
            if (fl >= 0) {
                if (fl != tbase) p0ok = true;                  // low end replaced by a frozen-mmax point
                p0c = e_pc; p0d = e_pd; cb = e_c; db = e_d;
                if (fl < lastl) { tc = e_nc; td = e_nd; } else { tc = ob; td = odb; }
                if (fl >= tbase + 2) { uc = e_ppc; ud = e_ppd; uok = true; }              // the point below the low end
                else if (fl == tbase + 1) { uc = oa; ud = oda; uok = oaok; }              // ... which may be the old low end
                else if (fl + 2 <= lastl) { uc = e_n2c; ud = e_n2d; uok = true; }         // first interval: two points above
                else if (fl + 1 == lastl) { uc = ob; ud = odb; uok = true; }
            } else {
                p0c = l_c; p0d = l_d; p0ok = true;
                if (G > 1) { tc = pl_c; td = pl_d; } else { tc = oa; td = oda; tok = oaok; }
                if (G > 2) { uc = pl2_c; ud = pl2_d; uok = true; }
            }
            {
                // Candidate root by inverse quadratic interpolation through the bracket ends and the
                // neighbouring point (offsets from the low end keep fp32 exact enough) and by the
                // secant.  Accept when the bracket is narrow AND the two agree (the secular function
                // is locally smooth, so the 3-point estimate is far better than their difference), or
                // when the bracket has shrunk to NEVILL's own tolerance (surfa.f:10,44).  Otherwise
                // subdivide again: near osculating modes Delta(c) is strongly curved and only a tight
                // bracket pins the root the reference finds.
                const float w = cb - p0c, sx = tc - p0c;
                // The estimates below are ratios of PRODUCTS of function values, formed with v_rcp_f32 - which returns 0 for
                // arguments beyond 2^126 and flushes results below 2^-126: with |Delta| ~ 1e19 .. 1e20 (water layer over soft
                // sediments at periods of a few seconds) the denominators (f1 - f0)(f1 - f2) ~ 1e38 .. 1e40 turned BOTH
                // three-point estimates into exactly 0, they "agreed", and the bracket's low end - a subdivision point up to
                // 1e-3 km/s from the root - was returned as the root (r04 soak: 1e-5 of random stacks, all team sizes below 16
                // lanes).  The values are brought to order one by a common power of two first (exact).
                const float fm = fmaxf(fabsf(p0d), fabsf(db));
                const int fex = (fm > 0.0f && fin(fm)) ? __builtin_amdgcn_frexp_expf(fm) : 0;
                const float f0 = ldexpf(p0d, -fex), f1 = ldexpf(db, -fex), f2 = ldexpf(td, -fex);
                ud = ldexpf(ud, -fex);
                auto qt = [](float a, float bq) { return a * __builtin_amdgcn_rcpf(bq); };
                float ts = qt(-f0 * w, f1 - f0);
                float t = qt(w * (f0 * f2), (f1 - f0) * (f1 - f2)) + qt(sx * (f0 * f1), (f2 - f0) * (f2 - f1));
                if (!(ts >= 0.0f)) ts = 0.0f;
                if (!(ts <= w)) ts = w;
                if (!p0ok) ts = 0.5f * w;                         // magnitudes not comparable: bisect
                const bool inside = p0ok && tok && (t >= 0.0f) && (t <= w);
                // Next to osculating modes the secular function bends sharply inside a bracket of a few 1e-4 km/s, and
                // inverse interpolation - every three-point estimate alike - then misses the root by several 1e-6 while
                // the estimates agree with each other (ragged fixture, 60 s: c off by 1.8e-6, which |dlnU/dlnc| = 560
                // turns into 1e-3 of U).  Such a bracket is subdivided again: the slope towards a neighbouring point must
                // be within a quarter of the slope across the bracket (ordinary brackets: a fraction of a percent).
                auto bends = [&](float xs, float fs) {                 // slopes compared without forming them
                    const float dm = f1 - f0;
                    const float dn = (xs > w) ? fs - f1 : f0 - fs, hn = (xs > w) ? xs - w : 0.0f - xs;
                    return !(fabsf(dn * w - dm * hn) <= 0.25f * fabsf(dm * hn));
                };
                const bool smooth = inside && !bends(sx, f2);
                bool agree = smooth && (fabsf(t - ts) <= A.atol);
                if (smooth && !agree && uok && !bends(uc - p0c, ud)) {
                    // The secant is only a second-order check: with a dozen evaluated points across the bracket a
                    // SECOND three-point estimate (same bracket ends, the neighbour on the other side) is the sharper
                    // witness - two cubically accurate estimates that agree to atol pin the root as well as another
                    // pass of subdivision would (deep stacks: half of the periods took that extra pass for the
                    // secant's sake, 28 of a stack's 95 passes instead of 19).
                    const float sx2 = uc - p0c, f3 = ud;
                    const float t2 = qt(w * (f0 * f3), (f1 - f0) * (f1 - f3)) + qt(sx2 * (f0 * f1), (f3 - f0) * (f3 - f1));
                    agree = (t2 >= 0.0f) && (t2 <= w) && (fabsf(t - t2) <= A.atol);
                }
                ++passes;                                          // hard bound: fp32 cannot resolve <1 ulp
                // ... and never across the KINK at the cut-off: a layer of finite thickness enters the secular function through
                // even functions of its vertical wavenumbers (cos, sin(x)/x, x sin(x)) and is smooth where c passes its P or S
                // velocity, but the half-space closure is LINEAR in sqrt|1 - c^2/b^2|: at the S velocity of the working stack's
                // half space the function behaves like sqrt|x|.  With that velocity among the points an estimate is built
                // from, all three-point estimates miss alike and still agree (ragged fixture, 60 s: root 5e-6 km/s below the
                // half space's S velocity; teams of 16 lanes accepted a 3.5e-5 bracket and came out 8e-6 off, 1e-3 of U at
                // |dlnU/dlnc| = 485; NEVILL - and teams of any other size - within 6e-7).  A bracket that reaches up to the
                // cut-off is subdivided until it no longer does (roots lie below it, calcul.f:191).
                bool accept = !(w > 1.0e-6f) || passes > 64;
                if (!accept && !(w > A.wtol) && agree) {
                    accept = !(W_B(mm_frozen - 1) <= cb * 1.000001f);
#ifdef SD_COUNT_KINK
                    if (j == 0 && A.amb_count && !accept) atomicAdd(A.amb_count + 1, 1);   // (developer statistics: refine passes added by the kink test)
#endif
                }
                if (accept) {
                    croot = p0c + (inside ? t : ts);
                    if (p0c >= 16.0f) fatal = true;                // NEVILL's 50 cycles, see above
                    else if (croot <= W_B(mm_frozen - 1)) {        // calcul.f:191
                        if (want_ratio) { st = ST_ELLIP; sub = 0; } else solved = true;
                    } else failed = true;
                }
            }
        } else if (st == ST_ELLIP) {
            if ((__ballot(ell_amb) & tmask) != 0ull) ell_flag = true;
            if (G == 1) {
                if (sub == 0) { r12 = val; sub = 1; }
                else { r12 = 0.5f * val / r12; solved = true; }
            } else {
                r12 = 0.5f * v1 / v0;                          // surfa.f:363
                solved = true;
            }
        }
        if (!EXACT && defer) {
            if (j == 0) A.fb_list[atomicAdd(A.fb_count, 1)] = (int)tg;
            defer = false; st = ST_DONE; solved = false; failed = false; fatal = false;
        }
        if (fatal) {
            nsolved = 0; k = 0; status = SURFDISP_NUMERIC; st = ST_DONE; ell_pend = false; solved = false; failed = false;
        }
        if (failed) {
            status = (k == 0) ? SURFDISP_NOROOT : SURFDISP_PARTIAL;
            st = ST_DONE;
        }
        if (LOCK) {
            // Lock step of the teams of a wavefront: with many teams per wavefront (16 of four lanes) SOME team is at its
            // refine pass or at the end of a period in nearly every pass, and the wavefront then runs those blocks for one
            // team in sixteen - team decisions and end-of-period block were 35 % of a ten-layer wavefront's time.  Here a team
            // with its bracket waits until no team of the wavefront scans any more, all refine together, and a team with its
            // root waits until all have theirs: one refine pass and one end-of-period block per period and wavefront.  A
            // waiting team evaluates nothing; each team's own sequence of evaluations - and so every result - is unchanged.
            if (solved) { st = ST_WEND; solved = false; }
            if (!__any(st == ST_SCAN) && st == ST_WREF) {
                st = ST_REFINE;
                if (bracket_phase(p0c, cb, mm_frozen) > A.phimulti) nevill_start();      // (see the bracket branch of the scan)
            }
            if (!__any(st == ST_SCAN || st == ST_WREF || st == ST_REFINE || st == ST_NEVILL || st == ST_NEVILL0 || st == ST_ELLIP) && st == ST_WEND)
                solved = true;
        }
#ifdef SD_WAVECLOCK
        const unsigned long long wb0 = __builtin_readcyclecounter();
#endif
        if (solved) {
            if (j == 0) {
                A.c[(size_t)k * B + b] = croot;                // period-major: coalesced across teams
                if (want_ratio) A.ratio[(size_t)k * B + b] = r12;
                // (exact kernel: negative - its ellipticity is final - with the same two fields, for the ellipticity kernels' replay)
                if (A.hist) A.hist[(size_t)k * B + b] = EXACT ? (int)(0x80000000u | (unsigned)nflat_cur | ((unsigned)mm_frozen << 16))
                                                              : (nflat_cur | (mm_frozen << 16) | (ell_flag ? 0x40000000 : 0));
            }
            ell_flag = false;
            nsolved = ++k;
            if (INDEP || k >= P) { st = ST_DONE; }
            else {
                T = A.per[k];
                mm_carry = mm_frozen;                          // mmax left by the last idrop=0 trial
#ifdef SD_DEBUG_TRIALS
                if (A.B == 1 && j == 0) printf("period %d starts: previous root %.7f, layers rebuilt for T = %.4f: %d of %d\n", k, croot, T, mm_carry, n);
#endif
                build(mm_carry);
                nflat_cur = mm_carry;
                b1top = W_B(0);
                p0c = 0.90f * croot;                           // calcul.f:143
                p0d = 0.0f; p0mm = 0; p0ok = false; first = true; passes = 0;
                coarse = false; fine_left = 1; q0ok = false;
                st = ST_SCAN;
                nodrop = no_drop_possible(p0c);
                defer = entry_overflow_risk(p0c);              // acted on at the end of the next pass
                if (CERT) coarse = nodrop;
            }
        }
#ifdef SD_WAVECLOCK
        wcyc_build += __builtin_readcyclecounter() - wb0;      // store of the root, next period's set-up, stack rebuild
#endif
    }
#ifdef SD_WAVECLOCK
    if (!EXACT && A.wclk && (threadIdx.x & 63) == 0) {
        const size_t w = (size_t)blockIdx.x * (SD_PHASE_BLOCK / 64) + (threadIdx.x >> 6);
        unsigned long long *o = A.wclk + 24 * w;
        o[0] = wclk0; o[1] = __builtin_amdgcn_s_memrealtime();
        o[2] = __builtin_readcyclecounter() - wcyc0; o[3] = wcyc_eval;
        o[4] = wcyc_build; o[5] = wpasses; o[6] = wcyc_pre;
        o[7] = wn_scan; o[8] = wn_refine; o[9] = wn_nevill; o[10] = wn_ellip; o[11] = wn_idle;
        o[12] = wtrip; o[13] = wlanelayers; o[14] = wlanes; o[15] = wsec[0];
        o[16] = wsec[1]; o[17] = wsec[2]; o[18] = wcyc_lean; o[19] = wn_lean; o[20] = wn_double;
    }
#endif
    if (INDEP) {
        // a failed period zeroes itself and every later one (calcul.f:203-219): the first failing
        // period index is reduced over the stack's teams; the finish kernel applies it
        if (team_valid && j == 0 && n >= 2 && status != SURFDISP_OK) {
            A.c[(size_t)k_own * B + b] = 0.0f;
            // -1: the secular function left the fp32 range somewhere in this stack (the finish kernel then
            // reports SURFDISP_NUMERIC, as the faithful mode does)
            atomicMin(&A.nsolved[b], status == SURFDISP_NUMERIC ? -1 : k_own);
        }
        return;
    }
    if (team_valid && j == 0) {
        if (n < 2) status = SURFDISP_BADMODEL;
        for (int q = nsolved; q < P; ++q) A.c[(size_t)q * B + b] = 0.0f;
        A.nsolved[b] = nsolved;
        if (A.status) A.status[b] = status;
    }
#undef M_AT
}

template <int KIND, int G, bool INDEP, bool FAST = false, bool EXACT = false>
__global__ __launch_bounds__(SD_PHASE_BLOCK) void surfdisp_phase_kernel(PhaseArgs A)
{
    phase_body<KIND, G, INDEP, FAST, EXACT>(A);
}

// ============================================================================= K1b: ellipticity
// The Rayleigh ellipticity of every solved (stack, period): 0.5 bb1(e3) / bb1(e2), the two extra recursions of
// DLTAR4(mup = 2) at the root (calcul.f:195, surfa.f:202-208,360-363), one lane per (stack, period) - full lanes, where the
// root search could give them two lanes of a team riding in the next period's scan pass and a second LDS working stack to
// read from (which cost deep stacks a workgroup per CU: 16 384 x L64, teams of 16: 51 KB -> 26 KB of LDS, three -> four
// workgroups per CU = the launch's 4 096 wavefronts in ONE round).
// The reference evaluates them on the working stack as phase 1 left it (COMMON /d/): only the first nflat layers are
// refreshed per period, the layer nflat - 1 in half-space form, deeper ones keep an earlier period's values - and the
// frozen mmax may reach into those.  The root search records (nflat, mmax) per solved period; this kernel replays the
// history: layer i carries the values of the LAST period k' <= k whose rebuild covered it (k' falls monotonically as i
// grows), with the same expressions the rebuild uses (layer_derive, rcp_nr), then steps both start vectors through
// ray_step / ray_close - the root search's own functions.
// r04: where the closure of either pass is the remainder of a cancellation (|value| below A.ell_ambig of its terms: soft
// sediments at c < 0.5 km/s, where the production recursion's ellipticity was good to 3e-4 .. 3e-3 only and cost 1e-4 of the
// group velocity) BOTH passes are evaluated again with the reference's own arithmetic (DLTAR4 statement by statement on the
// replayed working stack) - the value calcul.f:195 itself forms.  only_flagged: the root search computed the ellipticities
// itself (two-lane teams) and marked the (stack, period) pairs that need this (bit 30 of the history word).
__global__ __launch_bounds__(256) void surfdisp_ellip_kernel(EllipArgs A)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int B = A.B, P = A.P;
    if (idx >= (size_t)B * P) return;
    const int b = (int)(idx % B), k = (int)(idx / B);       // a wavefront = 64 stacks, one period: coalesced SoA reads
    const int n = A.nl[b];
    if (n < 2 || k >= A.nsolved[b]) return;                 // (the finish kernel writes 0 for unsolved periods)
    const int hk = A.hist[idx];
    if (hk < 0) return;                                      // computed by the exact fallback kernel itself
    if (A.only_flagged && !(hk & 0x40000000)) return;
    const int mmf = (hk >> 16) & 0x3fff;
    const size_t fs = (size_t)A.Lmax * B;
    const float c = A.c[idx], T = A.per[k];
    // the working stack as phase 1 left it, layer by layer (i = 0, 1, ... in order): the period whose rebuild last refreshed
    // layer i, and that rebuild's extent
    struct Replay { int kk, nflat; float lnT; };
    const Replay r0{k, hk & 0xffff, logf(1.0f / T)};
    auto layer = [&](int i, Replay &r) -> LayerV {
        while (r.nflat <= i && r.kk > 0) {                   // an earlier rebuild: period 0 refreshed all n layers
            --r.kk;
            const int h = A.hist[(size_t)r.kk * B + b];
            r.nflat = (h < 0) ? n : (h & 0xffff);
            r.lnT = logf(1.0f / A.per[r.kk]);
        }
        return layer_derive(layer_load(A.mdl, fs, (size_t)i * B + b), r.lnT, i == r.nflat - 1);
    };
    const int last = mmf - 1;
    float v2 = 0.0f, v3 = 0.0f;
    bool exact = A.only_flagged != 0;
    if (!exact) {
        const RTrial t = ray_trial(c, T);
        int kk = k;                                          // period whose rebuild last refreshed the layer at hand
        int nflat = hk & 0xffff;
        float lnT = r0.lnT;
        RState s2{}, s3{};
        float phi = 0.0f, rho_prev = 0.0f;
        RLyr y{};
        float rho_i = 0.0f;
        for (int i = 0; i <= last; ++i) {
            while (nflat <= i && kk > 0) {                   // an earlier rebuild: period 0 refreshed all n layers
                --kk;
                const int h = A.hist[(size_t)kk * B + b];
                nflat = (h < 0) ? n : (h & 0xffff);
                lnT = logf(1.0f / A.per[kk]);
            }
            const LayerV v = layer_derive(layer_load(A.mdl, fs, (size_t)i * B + b), lnT, i == nflat - 1);
            rho_prev = rho_i;
            rho_i = v.rho;
            y.sv = v.b; y.d = v.d;
            y.ia2 = wk_ia2(v.a);
            y.ib2 = wk_ib2(v.b);
            y.rat = (i > 0) ? wk_rat(rho_prev, rho_i) : 0.0f;
            if (i == 0) {
                const float irho0 = wk_irho(rho_i);
                s2 = ray_start(t, 2, irho0);
                s3 = ray_start(t, 3, irho0);
                if (last >= 1) { ray_step<true>(s2, t, y, 2, phi); ray_step<true>(s3, t, y, 3, phi); }
            } else if (i < last) {
                ray_step<false>(s2, t, y, 2, phi);
                ray_step<false>(s3, t, y, 3, phi);
            }
        }
        const float rp = (last >= 1) ? rho_prev : 0.0f;
        float m2 = 0.0f, m3 = 0.0f;
        v2 = ray_close(s2, t, y, rho_i, rp, 2, &m2); v3 = ray_close(s3, t, y, rho_i, rp, 3, &m3);
        // ... or where c is far below a layer's S velocity: g = 2 b^2 / c^2 of that layer is in the hundreds and the recursion's
        // u1 = g^2 b1 + 2 g h3 - h5 (as the reference's a11 .. a51, differently arranged) cancels inside the LAYER steps - soft
        // sediments over rock, c = 0.2 .. 0.4 km/s: the production ellipticity came out 3e-4 .. 4e-3 off the reference's (1e-4
        // .. 4e-4 of U) with an unremarkable closure.  The stack's largest flattened S velocity is the prep kernel's statistic.
        const float b2max = A.ovf ? 0.5f * __expf(0.25f * A.ovf[2 * (size_t)B + b]) : 0.0f;
        exact = (A.ell_ambig < 0.0f) ||
                ((A.ell_ambig > 0.0f) && (fabsf(v2) < A.ell_ambig * m2 || fabsf(v3) < A.ell_ambig * m3 || 2.0f * b2max > A.ell_gmax * c * c));
    }
    if (exact) {
        Replay r = r0;
        v2 = delta_rayleigh_ref_gen([&](int m) { const LayerV v = layer(m, r); return RefLyr{v.a, v.b, v.rho, v.d}; }, mmf, c, T, 2);
        r = r0;
        v3 = delta_rayleigh_ref_gen([&](int m) { const LayerV v = layer(m, r); return RefLyr{v.a, v.b, v.rho, v.d}; }, mmf, c, T, 3);
        if (A.amb_count) atomicAdd(A.amb_count + 1, 1);
    }
    A.ratio[idx] = 0.5f * v3 / v2;                           // surfa.f:363
}

// ================================================================================== K2: group
// sublayer bookkeeping shared by Rayleigh and Love (surfa.f:781-822 / 412-446): layers are split
// into ndiv equal sublayers with identical properties, so nothing is materialised -- a layer is
// visited with a repeat count.
struct Drop { int hs_layer; int nreg_hs; };

template <int KIND>
SD_HD __forceinline__ Drop drop_group(const float *__restrict__ mdl, size_t fs, int B, int b,
                                           int n, float lnT, float c, float T, int ndiv, bool water,
                                           float div)
{
    // surfa.f:853-866 (Rayleigh: compares a then b across the cut) / 475-487 (Love: b only).
    // Cuts can only happen at layer boundaries because sublayers of one layer are identical.
    const float dmax = FACT * T * c;
    float sum = 0.0f;
    Drop r; r.hs_layer = n - 1; r.nreg_hs = 0;
    LayerRaw nraw = layer_load(mdl, fs, (size_t)b);
    for (int jl = 0; jl < n; ++jl) {
        const LayerRaw raw = nraw;
        if (jl + 1 < n) nraw = layer_load(mdl, fs, (size_t)(jl + 1) * B + b);
        const LayerV v = layer_derive(raw, lnT, jl == n - 1);
        if (!(c < v.b)) continue;
        if (jl == n - 1) break;                                   // ii == mmax: keep the true half space
        const int nsub = (jl == 0 && water) ? 1 : ndiv;
        const float dsub = (ndiv > 1 && !(jl == 0 && water)) ? v.d / div : v.d;
        for (int s = 0; s < nsub; ++s) sum = sum + dsub;
        if (!(sum > dmax)) continue;
        const LayerV nx = layer_derive(nraw, lnT, jl + 1 == n - 1);
        bool lower, equal;
        if (KIND == 2) {
            lower = (nx.a < v.a) || (nx.a == v.a && nx.b < v.b);
            equal = (nx.a == v.a) && (nx.b == v.b);
        } else {
            lower = nx.b < v.b;
            equal = nx.b == v.b;
        }
        if (lower) { r.hs_layer = jl; r.nreg_hs = nsub - 1; break; }   // label 902: mmax = ii
        if (equal) continue;
        r.hs_layer = jl + 1; r.nreg_hs = 0; break;                     // label 90009: mmax = ii+1
    }
    return r;
}

// No cut possible: the walk above cuts only where its running sum of evanescent sublayer thicknesses exceeds
// dmax = FACT T c, and that sum cannot exceed the thickness of everything above the half space.  tot = sum |dfl| over
// the layers 0 .. n-2 (period-independent: one load and one add per layer, against nine loads, a layer_derive with two
// IEEE divisions and up to ndiv adds per layer of the walk); where tot (1 + 1e-4) <= dmax the walk returns {n - 1, 0},
// and so does drop_or_none without walking.  On 200 km stacks that is every period from ~15 s up.
// Why 1e-4 is enough.  The walk adds m = ndiv (n - 1) terms dsub = fl(d / div) in fp32, in layer order, over a SUBSET of
// the layers: m <= 99 for Rayleigh (ndiv <= 99 / (n - 1); 199 where ndiv = 1), m <= 5 x 199 = 995 for Love at
// SURFDISP_NLAY_MAX layers.  Its sum is at most sum |d| (1 + u)^m, u = 2^-24 (each dsub <= |d| / div (1 + u), each
// addition another (1 + u); terms of either sign: the error of a running sum is bounded by the sum of the magnitudes).
// tot, n - 1 <= 199 additions of the magnitudes, is at least sum |d| (1 - u)^(n - 2).  So the walk's sum is
// <= tot (1 + (m + n) u + ...) <= tot (1 + 7.2e-5) (1.8e-5 for Rayleigh), and the product tot (1 + 1e-4) rounds by one
// more u.  The test is one-sided: it only ever says "no cut" where the walk says so; anything else (a NaN included) walks.
#define SD_NO_DROP_SLACK 1.0e-4f
SD_HD __forceinline__ bool group_no_cut(const float *__restrict__ mdl, size_t fs, int B, int b, int n, float c, float T)
{
    float tot = 0.0f;
    for (int jl = 0; jl + 1 < n; ++jl) tot = tot + fabsf(mdl[F_DFL * fs + (size_t)jl * B + b]);
    return tot * (1.0f + SD_NO_DROP_SLACK) <= FACT * T * c;
}
template <int KIND>
SD_HD __forceinline__ Drop drop_or_none(const float *__restrict__ mdl, size_t fs, int B, int b,
                                             int n, float lnT, float c, float T, int ndiv, bool water,
                                             float div)
{
#ifndef SD_NO_DROP_SHORTCUT
    if (group_no_cut(mdl, fs, B, b, n, c, T)) return Drop{n - 1, 0};
#endif
    return drop_group<KIND>(mdl, fs, B, b, n, lnT, c, T, ndiv, water, div);
}

// Analytic partial derivatives of the phase velocity (the quantities REIGEN / LEIGEN form from their
// energy integrals and leave in COMMON /rar1/: surfa.f:1130-1135, 1180-1184, 1204-1207 / 509-512, 561-565, 581-583).
// The eigenproblem is solved for the attenuation-dispersed, earth-flattened layer values; the
// caller's derivatives are with respect to its own Vs, Vp, rho, so each layer carries the chain
// factors of calcul.f:122-126 and flat1.f:44-62:
//   b = b_ref (1 + qsq) f,  a = a_ref (1 + qsq 4/3 b_ref^2/a_ref^2) f,  rho = rho_ref r
// (KOut::raw, SURFDISP_KERN_REFCOORD: unit chain factors - the partials with respect to the flattened, attenuated layer
// values themselves, i.e. the reference's own numbers summed over a layer's sublayers; the water layer's share, which the
// reference does not form, is left out: what tests/golden/ref_partials.npz pins.)
//
// Where they go (r04).  A unit = one (stack, period) = one lane.  Every layer's share is written ONCE, unscaled, as soon as
// the sweep has it (a plain store: no zero fill, no read-modify-write; the share of the layer that also holds the half
// space is kept in three registers until the half-space terms are known); the common factor 1 / (dL/dk) - known only after
// the last layer - and the index of the deepest layer written go to two per-unit words, and the consumer applies them:
//   * scratch route (kernels workspace): layer-major scratch [3][Lmax][P*B] - the lanes of a wavefront (consecutive stacks,
//     one period) store consecutive words; surfdisp_kern_transpose_kernel reads it back through an LDS tile, multiplies by
//     the unit's factor, writes zeros for layers below the unit's half space / unsolved units, and stores whole rows of the
//     caller's [B][P][Lmax] arrays.  HBM traffic: scratch written once, read once, rows written once (r03: zero fill +
//     accumulate + scale, each a read-modify-write of the scratch, + the transposition: 7.2 x the rows).
//   * direct route (a workspace without the scratch): the same stores go to the caller's rows (stride 1) and the lane
//     itself scales / zero-fills its rows at the end - the same products, so both routes agree bit for bit.
struct KOut {
    float *b;                 // this unit's entry of layer 0 in the dc/dVs array; nullptr: no partials
    size_t stride;            // words between consecutive layers (uniform)
    ptrdiff_t off_a, off_r;   // BYTE offsets of the dc/dVp and dc/drho entries from the dc/dVs entry (uniform; 0: not wanted)
    int raw;                  // reference coordinates (see above)
    SD_HD void put(int i, float vb, float va, float vr) const
    {
        float *q = b + (size_t)i * stride;
        *q = vb;
        if (off_a) *reinterpret_cast<float *>(reinterpret_cast<char *>(q) + off_a) = va;
        if (off_r) *reinterpret_cast<float *>(reinterpret_cast<char *>(q) + off_r) = vr;
    }
};
// Eigenfunctions (the EIG instantiations; surfdisp_forward_eigen_device, K2d): the displacement-stress vector the sweep holds
// at the TOP of every caller layer i <= hs_layer - a knot of every split (fast_sublayers, the reference's ndiv) and of both
// Rayleigh paths - stored fp32 like the reference's real*4 COMMON /rar/ (surfa.f:389, 728), one plain store per component
// into a layer-major scratch [4][Lmax][P*B] (Love: [2]), the layout of the partials' scratch: the lanes of a wavefront
// write consecutive words.  Entry (component q, layer i) of this unit sits at p[q * plane + i * stride].
struct EOut {
    float *p;
    size_t stride, plane;
    SD_HD void put(int i, float ur, float uz, float tz, float tr) const
    {
        float *q = p + (size_t)i * stride;
        q[0] = ur; q[plane] = uz; q[2 * plane] = tz; q[3 * plane] = tr;
    }
    SD_HD void put2(int i, float ut, float tq) const
    {
        float *q = p + (size_t)i * stride;
        q[0] = ut; q[plane] = tq;
    }
};
// ... and per unit: the divisor of the stored values (Rayleigh 1: the sweep is normalised to uz = 1 at the top of the first
// solid layer; Love: ut at the top, known only after the last layer, surfa.f:580-581), the deepest layer written (-1: none -
// the degenerate exits leave zero rows and zero integrals) and the three sums exactly as the U expression consumes them.
struct EUnit { float div; int hs; float i0, i1, i2; };
struct K3 { float b, a, r; };
struct Chain { float dbdb, dadb, dada, rfac; };
SD_HD __forceinline__ Chain chain_of(const LayerRaw &r, float lnT, bool is_halfspace, bool raw)
{
    if (raw) return Chain{1.0f, 0.0f, 1.0f, 1.0f};
    const float qsq = r.qs * lnT / PI_REF;
    const float qpq = qsq * 1.33333333f * (r.b_ref * r.b_ref) / (r.a_ref * r.a_ref);
    const float vfac = is_halfspace ? r.hsf : r.dif;
    Chain ch;
    ch.dbdb = (1.0f + qsq) * vfac;
    ch.dadb = 2.66666667f * qsq * (r.b_ref / r.a_ref) * vfac;
    ch.dada = (1.0f - qpq) * vfac;
    ch.rfac = is_halfspace ? r.hsr : r.qqq;
    return ch;
}
// One layer's share from its six energy integrals (surfa.f:1110-1121, summed over the layer's sublayers) -> dL/d(lambda,
// mu, rho) (surfa.f:1130-1132) -> dc/d(b, a, rho) of the flattened layer, still to be divided by dL/dk (surfa.f:1133-1135)
// -> the caller's layer.  Everything that depends on the layer alone - 2 rho b c/k and the chain factors - is folded into
// four coefficients when the layer is entered (KC: the layer's raw values need not stay in registers across its RK4 steps).
// fp32: the integrals are fp32 Boole sums; 1e-7 of their largest term is 1e-6 of a period's largest partial.
struct KC { float b1, b2, a, r; };
SD_HD __forceinline__ KC kern_coef(const LayerRaw &raw, const LayerV &v, float lnT, bool is_halfspace, float cw, bool rawc)
{
    const Chain ch = chain_of(raw, lnT, is_halfspace, rawc);
    const float rc2 = 2.0f * v.rho * cw;                     // 2 rho c / k
    return KC{rc2 * v.b * ch.dbdb, rc2 * v.a * ch.dadb, rc2 * v.a * ch.dada, cw * ch.rfac / v.rho};
}
// KR: the type the six sums are carried and combined in.  dc/drho is the difference of the kinetic and the two elastic
// terms, which cancel to ~1e-3 of their size (equipartition): combined in fp32 it came out 6e-4 of a period's peak off
// the reference's value (tests/golden/ref_partials.npz) - the reference carries them DOUBLE PRECISION (surfa.f:717-722).
typedef double KR;
SD_HD __forceinline__ K3 kern_layer_rayleigh(const KC &kc, float rho, float xlamb, float xmu, float wvno, float wvnosq,
                                             float omegsq, KR dmmr, KR dmmz, KR drsz, KR dzsr, KR smmz, KR smmr)
{
    const KR two = 2, k2 = wvnosq, tk = 2.0f * wvno;
    const KR dldl = -k2 * dmmr + tk * drsz - smmz;
    const KR dldm = -k2 * (two * dmmr + dmmz) - tk * dzsr - (two * smmz + smmr);
    const KR dldr = (KR)omegsq * (dmmr + dmmz);
    return K3{(float)((KR)kc.b1 * (dldm - two * dldl) + (KR)kc.b2 * dldl), (float)((KR)kc.a * dldl),
              (float)((KR)kc.r * ((KR)rho * dldr + (KR)xlamb * dldl + (KR)xmu * dldm))};
}

// ---- Rayleigh, surfa.f:714-1192 ---------------------------------------------------------------
struct RCoef { float a12, a13, a21, a24, a31, a34, a42, a43, ddz; };

struct RInt {                       // energy integrals, fp64 accumulators (reference: fp32 sumi*)
    double i0, i1, i2;
};

// One RK4 step of a constant-coefficient linear system is a fixed linear map.  With the state split
// as x = (ur, tz), w = (uz, tr) the system matrix is block anti-diagonal (x' = M1 w, w' = M2 x), so
//   P = I + k1 A + k2 A^2 + k3 A^3 + k4 A^4 = [[I + k2 N1 + k4 N1^2,  k1 M1 + k3 N1 M1],
//                                             [k1 M2 + k3 N2 M2,  I + k2 N2 + k4 N2^2]],
// N1 = M1 M2, N2 = M2 M1.  k1..k4 are formed from the reference's fp32 weights exactly as its stage
// recursion combines them (surfa.f:764-771, 955-968), so P reproduces the reference's step to fp64
// rounding at a quarter of the arithmetic; all sublayers of a layer share it.
struct M2x2 { double a, b, c, d; };     // [[a b],[c d]]
SD_HD __forceinline__ M2x2 mm(const M2x2 &x, const M2x2 &y)
{
#pragma clang fp contract(off)
    M2x2 r;
    r.a = fma(x.a, y.a, x.b * y.c); r.b = fma(x.a, y.b, x.b * y.d);
    r.c = fma(x.c, y.a, x.d * y.c); r.d = fma(x.c, y.b, x.d * y.d);
    return r;
}
// x y + u v, one multiply and three fma per element
SD_HD __forceinline__ M2x2 mm2(const M2x2 &x, const M2x2 &y, const M2x2 &u, const M2x2 &v)
{
#pragma clang fp contract(off)
    M2x2 r;
    r.a = fma(x.a, y.a, fma(x.b, y.c, fma(u.a, v.a, u.b * v.c))); r.b = fma(x.a, y.b, fma(x.b, y.d, fma(u.a, v.b, u.b * v.d)));
    r.c = fma(x.c, y.a, fma(x.d, y.c, fma(u.c, v.a, u.d * v.c))); r.d = fma(x.c, y.b, fma(x.d, y.d, fma(u.c, v.b, u.d * v.d)));
    return r;
}
SD_HD __forceinline__ M2x2 madd(const M2x2 &x, const M2x2 &y)
{
    M2x2 r; r.a = x.a + y.a; r.b = x.b + y.b; r.c = x.c + y.c; r.d = x.d + y.d; return r;
}
struct RProp { M2x2 p11, p12, p21, p22; };

SD_HD __forceinline__ RProp make_prop(const RCoef &q)
{
#pragma clang fp contract(off)
    const double wh = (double)(0.5f * q.ddz), w1 = (double)(1.0f * q.ddz);
    const double t6 = (double)((1.0f / 6.0f) * q.ddz), t3 = (double)((1.0f / 3.0f) * q.ddz);
    const double k1 = (t6 + t3) + (t3 + t6);
    const double k2 = (t3 * wh + t3 * wh) + t6 * w1;
    const double k3 = t3 * wh * wh + t6 * w1 * wh;
    const double k4 = t6 * w1 * wh * wh;
    const M2x2 m1 = {(double)q.a31, (double)q.a34, (double)q.a21, (double)q.a24};
    const M2x2 m2 = {(double)q.a13, (double)q.a12, (double)q.a43, (double)q.a42};
    // One block of P at a time (register pressure: this kernel sits at the 168-VGPR boundary of three
    // wavefronts per SIMD).  N^2 of a 2x2 matrix is tr(N) N - det(N) I (Cayley-Hamilton), so
    //   I + k2 N + k4 N^2 = (1 - k4 det) I + (k2 + k4 tr) N      and      k1 M + k3 N M = (k1 I + k3 N) M
    // need no explicit N^2 and N M products (fp64 runs at half rate here).
    RProp P;
    auto diag_block = [&](const M2x2 &nn) -> M2x2 {
        const double tr = nn.a + nn.d;
        const double det = fma(nn.a, nn.d, -(nn.b * nn.c));
        const double al = fma(k4, tr, k2), be = fma(-k4, det, 1.0);
        return M2x2{fma(al, nn.a, be), al * nn.b, al * nn.c, fma(al, nn.d, be)};
    };
    auto off_block = [&](const M2x2 &nn, const M2x2 &m) -> M2x2 {
        const M2x2 q = {fma(k3, nn.a, k1), k3 * nn.b, k3 * nn.c, fma(k3, nn.d, k1)};
        return mm(q, m);
    };
    {
        const M2x2 n1 = mm(m1, m2);
        P.p11 = diag_block(n1);
        P.p12 = off_block(n1, m1);
    }
    {
        const M2x2 n2 = mm(m2, m1);
        P.p22 = diag_block(n2);
        P.p21 = off_block(n2, m2);
    }
    return P;
}
// Closed-form powers of P.  Every polynomial in A has the block form of P above, so
//   P^m = [[F(N1), G(N1) M1], [G(N2) M2, F(N2)]],   F(N) = f0 I + f1 N,  G(N) = g0 I + g1 N:
// N1 and N2 share their trace t and determinant d, and every polynomial in N reduces modulo N^2 = t N - d I.  P^m is
// carried as its four scalars and multiplied as (F, G)(F', G') = (F F' + N G G', F G' + G F'), each product reduced with
// the same rule: no division, and valid when the two eigenvalues of N coincide.
struct RPow { double f0, f1, g0, g1; };
struct RBase { M2x2 m1, m2, n1, n2; double t, d; RPow p; };   // one layer: the blocks of A, N1, N2, and P's scalars
SD_HD __forceinline__ RBase make_base(const RCoef &q)
{
#pragma clang fp contract(off)
    // k1..k4, M1, M2, t, d and P's scalars exactly as make_prop forms them
    const double wh = (double)(0.5f * q.ddz), w1 = (double)(1.0f * q.ddz);
    const double t6 = (double)((1.0f / 6.0f) * q.ddz), t3 = (double)((1.0f / 3.0f) * q.ddz);
    const double k1 = (t6 + t3) + (t3 + t6);
    const double k2 = (t3 * wh + t3 * wh) + t6 * w1;
    const double k3 = t3 * wh * wh + t6 * w1 * wh;
    const double k4 = t6 * w1 * wh * wh;
    RBase r;
    r.m1 = M2x2{(double)q.a31, (double)q.a34, (double)q.a21, (double)q.a24};
    r.m2 = M2x2{(double)q.a13, (double)q.a12, (double)q.a43, (double)q.a42};
    r.n1 = mm(r.m1, r.m2);
    r.n2 = mm(r.m2, r.m1);
    r.t = r.n1.a + r.n1.d;
    r.d = fma(r.n1.a, r.n1.d, -(r.n1.b * r.n1.c));
    r.p = RPow{fma(-k4, r.d, 1.0), fma(k4, r.t, k2), k1, k3};
    return r;
}
// x y for two polynomials reduced modulo N^2 = t N - d I: (x0 y0 - d x1 y1) + (x0 y1 + x1 y0 + t x1 y1) N
SD_HD __forceinline__ RPow pow_mul(const RPow &x, const RPow &y, double t, double d)
{
#pragma clang fp contract(off)
    const double ff = x.f1 * y.f1, gg = x.g1 * y.g1, fg = fma(x.f1, y.g1, x.g1 * y.f1);
    // F F' and G G' (reduced), then F F' + N G G' with N (g0 + g1 N) = -d g1 + (g0 + t g1) N
    const double a0 = fma(x.f0, y.f0, -d * ff), a1 = fma(x.f0, y.f1, fma(x.f1, y.f0, t * ff));
    const double b0 = fma(x.g0, y.g0, -d * gg), b1 = fma(x.g0, y.g1, fma(x.g1, y.g0, t * gg));
    RPow r;
    r.f0 = fma(-d, b1, a0);
    r.f1 = fma(t, b1, a1 + b0);
    r.g0 = fma(x.f0, y.g0, fma(x.g0, y.f0, -d * fg));
    r.g1 = fma(x.f0, y.g1, fma(x.f1, y.g0, fma(x.g0, y.f1, fma(x.g1, y.f0, t * fg))));
    return r;
}
SD_HD __forceinline__ RPow pow_sq(const RPow &x, double t, double d)
{
#pragma clang fp contract(off)
    const double ff = x.f1 * x.f1, gg = x.g1 * x.g1, fg = x.f1 * x.g1;
    const double a0 = fma(x.f0, x.f0, -d * ff), a1 = fma(2.0 * x.f0, x.f1, t * ff);
    const double b0 = fma(x.g0, x.g0, -d * gg), b1 = fma(2.0 * x.g0, x.g1, t * gg);
    RPow r;
    r.f0 = fma(-d, b1, a0);
    r.f1 = fma(t, b1, a1 + b0);
    r.g0 = 2.0 * fma(x.f0, x.g0, -d * fg);
    r.g1 = 2.0 * fma(x.f0, x.g1, fma(x.f1, x.g0, t * fg));
    return r;
}
// P^(4 nreg), nreg >= 1: two squarings to P^4 (one sublayer), then binary powering (nreg = 5: P^16 P^4)
SD_HD __forceinline__ RPow pow_sublayers(const RBase &L, int nreg)
{
    RPow q = pow_sq(pow_sq(L.p, L.t, L.d), L.t, L.d);
    RPow r = (nreg & 1) ? q : RPow{1.0, 0.0, 0.0, 0.0};   // (a product with the identity is exact)
    for (int e = nreg >> 1; e > 0; e >>= 1) {
        q = pow_sq(q, L.t, L.d);
        if (e & 1) r = pow_mul(r, q, L.t, L.d);
    }
    return r;
}
// the 16 entries of P^m from its scalars
SD_HD __forceinline__ RProp pow_expand(const RBase &L, const RPow &x)
{
#pragma clang fp contract(off)
    RProp P;
    P.p11 = M2x2{fma(x.f1, L.n1.a, x.f0), x.f1 * L.n1.b, x.f1 * L.n1.c, fma(x.f1, L.n1.d, x.f0)};
    P.p22 = M2x2{fma(x.f1, L.n2.a, x.f0), x.f1 * L.n2.b, x.f1 * L.n2.c, fma(x.f1, L.n2.d, x.f0)};
    P.p12 = mm(M2x2{fma(x.g1, L.n1.a, x.g0), x.g1 * L.n1.b, x.g1 * L.n1.c, fma(x.g1, L.n1.d, x.g0)}, L.m1);
    P.p21 = mm(M2x2{fma(x.g1, L.n2.a, x.g0), x.g1 * L.n2.b, x.g1 * L.n2.c, fma(x.g1, L.n2.d, x.g0)}, L.m2);
    return P;
}
SD_HD __forceinline__ RProp prop_sq(const RProp &P)
{
    RProp Q;
    Q.p11 = mm2(P.p11, P.p11, P.p12, P.p21);
    Q.p12 = mm2(P.p11, P.p12, P.p12, P.p22);
    Q.p21 = mm2(P.p21, P.p11, P.p22, P.p21);
    Q.p22 = mm2(P.p21, P.p12, P.p22, P.p22);
    return Q;
}
// v = (ur, uz, tz, tr)
SD_HD __forceinline__ void prop_apply(const RProp &P, double v[4])
{
#pragma clang fp contract(off)
    const double ur = v[0], uz = v[1], tz = v[2], tr = v[3];
    // one multiply and three fused multiply-adds per row (fp64 runs at half rate: the applications of P
    // are most of this kernel's time); every sweep uses this same routine, so they stay bit-consistent
    v[0] = fma(P.p11.a, ur, fma(P.p11.b, tz, fma(P.p12.a, uz, P.p12.b * tr)));
    v[2] = fma(P.p11.c, ur, fma(P.p11.d, tz, fma(P.p12.c, uz, P.p12.d * tr)));
    v[1] = fma(P.p21.a, ur, fma(P.p21.b, tz, fma(P.p22.a, uz, P.p22.b * tr)));
    v[3] = fma(P.p21.c, ur, fma(P.p21.d, tz, fma(P.p22.c, uz, P.p22.d * tr)));
}

// Sublayers of the fast path's energy-integral sweep.  The reference splits every layer into ndiv = min(5, 99/(n-1))
// sublayers of 4 RK4 steps whatever the layer's wavelength (surfa.f:781-822); the fast path (combined solution, one
// 4-vector) integrates a layer's depth H in n' <= nreg equal sublayers, the fewest with lambda h <= SD_GROUP_LAMH,
// h = H / (4 n') the RK4 step and lambda = k max(|1 - c^2/a^2|, |1 - c^2/b^2|)^(1/2) the layer's largest |eigenvalue|.
// Error per step (fp32 knots: integrands rounded to 6e-8 relative):
//   RK4, local:  (lambda h)^5 / 120                     0.05: 2.6e-9   (<= 20 steps per layer: <= 5e-8)
//   Boole, one sublayer of an e^(2 lambda z) integrand:  (8/945) (2 lambda h)^6 / 4 = 0.135 (lambda h)^6   0.05: 2.1e-9
// both below the fp32 rounding of a single knot's integrand.  (lambda H)^2 = H^2 max(|k^2 - w^2/a^2|, |k^2 - w^2/b^2|)
// from the step's own coefficients (a21 = -w^2 rho, a12 = 1/(rho a^2), a34 = 1/(rho b^2)): no square root, no division.
// A layer that needs all nreg sublayers keeps the reference's step bit for bit.  SD_GROUP_LAMH <= 0: the reference's
// split everywhere.  The fast path's fit (MODE 0) steps the same split as its sweep (own = true in both, group_rayleigh);
// the robust path (MODE 1 and the two-vector sweep) keeps the reference's split.
#ifndef SD_GROUP_LAMH
#define SD_GROUP_LAMH 0.05f
#endif
#ifndef SD_GROUP_OWN_CANCEL
#define SD_GROUP_OWN_CANCEL 1.0e5    // largest fit cancellation at which the fast path keeps its own split (group_rayleigh)
#endif
SD_HD __forceinline__ int fast_sublayers(const RCoef &q, float wvnosq, float dsub, int nreg)
{
    if (!(SD_GROUP_LAMH > 0.0f)) return nreg;
    const float lam2 = fmaxf(fabsf(fmaf(q.a21, q.a12, wvnosq)), fabsf(fmaf(q.a21, q.a34, wvnosq)));
    const float H = dsub * (float)nreg;
    const float x = lam2 * H * H;                                     // (lambda H)^2
    constexpr float t = 16.0f * SD_GROUP_LAMH * SD_GROUP_LAMH;        // (4 lambda h)^2 at the bound, n' = 1
    int m = 1;
#pragma unroll
    for (int i = 1; i < 5; ++i) m += (x > t * (float)(i * i)) ? 1 : 0;
    return m < nreg ? m : nreg;
}

// integrate both solutions from the half space to the surface.  INTEG = false: only the surface
// values are wanted, so a layer is one application of P^(4 nreg).  INTEG = true: step by step, and
// accumulate the Boole energy integrals of the combined solution (xnorm*y + z)/bb
// (surfa.f:1087-1129).  The two sweeps agree to fp64 rounding (~1e-15 relative), far inside what the
// ~1e6 cancellation of the combination needs.
// MODE 0: surface values only, one application of the closed-form P^(4 nreg) per layer (fast path's fit);
// MODE 1: surface values only, four applications of P per sublayer - bit-identical to what MODE 2
//         computes, which the robust path needs (see group_rayleigh);
// MODE 2: energy integrals.  two_vec = false: z[] is the combined solution itself (fast path);
//         two_vec = true: y[] and z[] are stepped separately and combined at every knot with the
//         fitted xnorm / bb, exactly like the reference's stored knots (surfa.f:1092-1095).
// EIG (MODE 2): also store the combined vector at the top of every layer the sweep steps through (EOut).
//
// LStash: a lane's own copy of what the fit (MODE 0) derives for every layer it steps through and the later sweeps
// (MODE 1, MODE 2) would derive again, bit for bit, from nine loads, layer_derive's two IEEE divisions and the IEEE
// reciprocals 1 / (lambda + 2 mu) and 1 / mu: rho, mu, lambda and the two reciprocals, word f of layer jl at
// p[(jl * SD_STASH_W + f) * str] (the group kernel: dynamic LDS, str = 256 lanes, p = base + lane - lane-private, one
// bank per lane).  Only values that do not depend on the sweep's split (own, nstep) are kept: the fit may run twice, and
// writes the same words both times.  A liquid layer, which the sweeps skip before they derive anything else, is marked
// by SD_STASH_LIQUID in its first word: a quiet NaN with a payload, which no arithmetic on the finite values the prep
// kernel lets through can produce (operations on finite operands give the default NaN, payload zero) - so no derived rho
// is mistaken for it.  p == nullptr: every sweep derives its own values (the KERN sweep, which needs the raw layer for
// its chain factors, always does).
#define SD_STASH_W 5
#define SD_STASH_LIQUID 0x7fc0dead
struct LStash { float *p; int str; };
template <int MODE, bool KERN = false, bool EIG = false, bool STASH = false>
SD_HD __forceinline__ void rayleigh_sweep(const float *__restrict__ mdl, size_t fs, int B, int b,
                                               int n, float lnT, int ndiv, bool water, float div,
                                               const Drop dr, float wvno, float wvnosq, float omegsq,
                                               double y[4], double z[4], bool do_y, bool own,
                                               double xnorm, double bbn, RInt &acc,
                                               const KOut ko = KOut{nullptr, 1, 0, 0, 0}, float cw = 0.0f, K3 *hold = nullptr,
                                               bool *shorter = nullptr, const EOut eo = EOut{nullptr, 1, 0},
                                               LStash *st = nullptr)
{
#pragma clang fp contract(off)   // both sweeps must see identical coefficients
    // (STASH: the instantiations that may be handed a stash - the others compile to the code they were without it)
    const bool keep = STASH && (MODE == 0) && st && st->p;          // the fit: leave the layer values for the sweeps
    const bool kept = STASH && (MODE != 0) && !KERN && st && st->p; // a later sweep: take them
#ifdef SD_SWEEP_PROBE
    SD_SWEEP_PROBE(MODE, own, kept);                                // host test builds only (tests/hostcheck/trimscheck.hip)
#endif
    LayerRaw nraw{};
    if (!kept) nraw = layer_load(mdl, fs, (size_t)dr.hs_layer * B + b);
    for (int jl = dr.hs_layer; jl >= 0; --jl) {
        const LayerRaw raw = nraw;
        if (!kept && jl > 0) nraw = layer_load(mdl, fs, (size_t)(jl - 1) * B + b);   // in flight during this layer
        const int nsub = (jl == 0 && water) ? 1 : ndiv;
        const int nreg = (jl == dr.hs_layer) ? dr.nreg_hs : nsub;
        if (nreg <= 0) continue;
        LayerV v;
        float xmu, xlamb;
        RCoef q;
        if (kept) {
            const float *sp = st->p + (size_t)(jl * SD_STASH_W) * st->str;
            v.rho = sp[0];
            if (__builtin_bit_cast(uint32_t, v.rho) == (uint32_t)SD_STASH_LIQUID) continue;   // water (no partials on this path: nothing to put)
            v.a = 0.0f; v.b = 0.0f;                                  // (unused from here on without KERN)
            v.d = mdl[F_DFL * fs + (size_t)jl * B + b];              // (a stepped layer is never the true half space: d = dfl)
            xmu = sp[st->str]; xlamb = sp[2 * st->str];
            q.a12 = sp[3 * st->str]; q.a34 = sp[4 * st->str];
        } else {
            v = layer_derive(raw, lnT, jl == n - 1);
            if (v.b <= 0.0f) {                                       // water: surfa.f:930
                if (MODE == 2 && KERN && jl > 0) ko.put(jl, 0.0f, 0.0f, 0.0f);   // (the top layer's entry: group_rayleigh)
                if (keep) st->p[(size_t)(jl * SD_STASH_W) * st->str] = __builtin_bit_cast(float, (uint32_t)SD_STASH_LIQUID);
                continue;
            }
            xmu = v.rho * v.b * v.b;                                 // surfa.f:831-832
            xlamb = v.rho * (v.a * v.a - 2.0f * v.b * v.b);
            q.a12 = 1.0f / (xlamb + 2.0f * xmu);
            q.a34 = 1.0f / xmu;
            if (keep) {
                float *sp = st->p + (size_t)(jl * SD_STASH_W) * st->str;
                sp[0] = v.rho; sp[st->str] = xmu; sp[2 * st->str] = xlamb;
                sp[3 * st->str] = q.a12; sp[4 * st->str] = q.a34;
            }
        }
        float dsub = (ndiv > 1 && !(jl == 0 && water)) ? v.d / div : v.d;
        KC kc{};
        if (MODE == 2 && KERN) kc = kern_coef(raw, v, lnT, jl == n - 1, cw, ko.raw != 0);
        q.a13 = wvno * xlamb * q.a12;
        q.a21 = -omegsq * v.rho;
        q.a24 = wvno; q.a31 = -wvno;
        q.a42 = -q.a13;
        q.a43 = q.a21 + 4.0f * wvnosq * xmu * (xlamb + xmu) * q.a12;
        int nstep = nreg;                                            // sublayers this sweep steps through the layer
        if (MODE != 1 && own) {                                      // fast path (its fit and its sweep): its own split
            nstep = fast_sublayers(q, wvnosq, dsub, nreg);
            if (nstep < nreg) {
                dsub = (dsub * (float)nreg) / (float)nstep;
                if (shorter) *shorter = true;                        // (the fit: some layer left the reference's split)
            }
        }
#ifdef SD_SPLIT_PROBE
        if (MODE == 2 && !do_y) SD_SPLIT_PROBE(nreg, nstep);         // host test builds only (tests/hostcheck/splitcheck.hip)
#endif
        q.ddz = -dsub / (4.0f * 1.0f);
        if (MODE == 0) {
            const RBase L = make_base(q);
            const RProp Pm = pow_expand(L, pow_sublayers(L, nstep));  // all the layer's sublayers at once
            if (do_y) prop_apply(Pm, y);
            prop_apply(Pm, z);
            continue;
        }
        const RProp P = make_prop(q);
        if (MODE == 1) {
            for (int s = 0; s < nreg; ++s) {
#pragma unroll
                for (int kk = 3; kk >= 0; --kk) {
                    if (do_y) prop_apply(P, y);
                    prop_apply(P, z);
                }
            }
            continue;
        }
        const bool two_vec = do_y;
        const float dz = dsub / 4.0f;
        const float l2m = xlamb + 2.0f * xmu;
        const float ixmu = q.a34, il2m = q.a12;       // 1/mu, 1/(lambda+2mu): already formed above
        float f_mr[5], f_mz[5], f_rz[5], f_zr[5];
        constexpr bool kern = KERN;
        KR k_mr = 0, k_mz = 0, k_rz = 0, k_zr = 0, k_sz = 0, k_sr = 0;   // this layer's sums
        float f_sz[5], f_sr[5];
        const double ibb = 1.0 / bbn;
        float e_ur = 0.0f, e_uz = 0.0f, e_tz = 0.0f, e_tr = 0.0f;    // (EIG) the last knot's vector
        auto knot = [&](int kk) {
            // fast path: z[] is the combined, normalised solution (xnorm*y + z)/bb itself;
            // robust path: combine the separately integrated solutions at the knot
            float aur, auz, atz, atr;
            if (two_vec) {
                aur = (float)((xnorm * y[0] + z[0]) * ibb); auz = (float)((xnorm * y[1] + z[1]) * ibb);
                atz = (float)((xnorm * y[2] + z[2]) * ibb); atr = (float)((xnorm * y[3] + z[3]) * ibb);
            } else {
                aur = (float)z[0]; auz = (float)z[1]; atz = (float)z[2]; atr = (float)z[3];
            }
            if constexpr (EIG) { e_ur = aur; e_uz = auz; e_tz = atz; e_tr = atr; }
            const float durdz = atr * ixmu - wvno * auz;
            const float duzdz = (atz + wvno * xlamb * aur) * il2m;
            f_mr[kk] = aur * aur; f_mz[kk] = auz * auz;
            f_rz[kk] = aur * duzdz; f_zr[kk] = auz * durdz;
            if (kern) {
                f_sz[kk] = duzdz * duzdz; f_sr[kk] = durdz * durdz;
            }
        };
        for (int s = 0; s < nstep; ++s) {
            // bottom knot: the top knot of the sublayer below when it belongs to the same layer
            if (s == 0) knot(4);
            else { f_mr[4] = f_mr[0]; f_mz[4] = f_mz[0]; f_rz[4] = f_rz[0]; f_zr[4] = f_zr[0];
                   if (kern) { f_sz[4] = f_sz[0]; f_sr[4] = f_sr[0]; }
            }
#pragma unroll
            for (int kk = 3; kk >= 0; --kk) {
                if (two_vec) prop_apply(P, y);
                prop_apply(P, z);
                knot(kk);
            }
            const float hq = dz / 22.5f;
#define SD_BOOLE(v) (hq * (7.0f * (v[0] + v[4]) + 32.0f * (v[1] + v[3]) + 12.0f * v[2]))
            const float dmmr = SD_BOOLE(f_mr), dmmz = SD_BOOLE(f_mz);
            const float drsz = SD_BOOLE(f_rz), dzsr = SD_BOOLE(f_zr);
            if (kern) {
                k_mr += dmmr; k_mz += dmmz; k_rz += drsz; k_zr += dzsr;
                k_sz += SD_BOOLE(f_sz); k_sr += SD_BOOLE(f_sr);
            }
#undef SD_BOOLE
            // the sublayer's contributions in fp32 as in the reference (surfa.f:1126-1128); only the
            // running sums are fp64 (fp64 arithmetic runs at half rate)
            acc.i0 += (double)(v.rho * (dmmr + dmmz));
            acc.i1 += (double)(l2m * dmmr + xmu * dmmz);
            acc.i2 += (double)(xmu * dzsr - xlamb * drsz);
        }
        // the layer's last knot (kk = 0 of its last sublayer) is the top of layer jl
        if constexpr (EIG) eo.put(jl, e_ur, e_uz, e_tz, e_tr);
        if (kern) {
            const K3 sh = kern_layer_rayleigh(kc, v.rho, xlamb, xmu, wvno, wvnosq, omegsq, k_mr, k_mz, k_rz, k_zr, k_sz, k_sr);
            if (jl == dr.hs_layer) *hold = sh;                       // the half-space terms join it (group_rayleigh)
            else ko.put(jl, sh.b, sh.a, sh.r);
        }
    }
}

#ifdef SD_COUNT_RESTARTS
// development build (make variant EXTRA=-DSD_COUNT_RESTARTS, scripts/restart_count.py): lanes and wavefronts whose fast fit
// restarts, read with surfdisp_dev_restart_count
__device__ unsigned long long sd_restart_count[2];
#endif

template <bool KERN = false, bool EIG = false, bool STASH = false>
SD_HD float group_rayleigh(const float *__restrict__ mdl, size_t fs, int B, int b, int n,
                                float T, float c, float ratio, double *dbg = nullptr,
                                const KOut ko = KOut{nullptr, 1, 0, 0, 0}, float *kscale = nullptr, int *khs = nullptr,
                                const EOut eo = EOut{nullptr, 1, 0}, EUnit *eu = nullptr, LStash *st = nullptr)
{
#pragma clang fp contract(off)
    const float lnT = logf(1.0f / T);
    int ndiv = 5;
    const int ivre = 99 / (n - 1);                                    // surfa.f:783-784
    if (ndiv > ivre) ndiv = ivre;
    if (ndiv < 1) ndiv = 1;
    const float div = (float)ndiv;
    const LayerV top = layer_at(mdl, fs, (size_t)b, lnT, false);
    const bool water = (ndiv > 1) ? (top.b <= 0.1e-10f) : false;      // jj=2 only when splitting
    const bool wet = !(top.b > 0.0f);
    const Drop dr = drop_or_none<2>(mdl, fs, B, b, n, lnT, c, T, ndiv, water, div);
    const float wvno = 6.2831853072f / (c * T);
    const float wvnosq = wvno * wvno;
    const float omega = 6.2831853072f / T;
    const float omegsq = omega * omega;
    RInt acc; acc.i0 = 0.0; acc.i1 = 0.0; acc.i2 = 0.0;
    float tzz = 0.0f;
    const float cw = c / wvno;                                        // (KERN) c / k
    K3 hold{0.0f, 0.0f, 0.0f};                                        // (KERN) share of the layer that holds the half space
    if (KERN) { *kscale = 0.0f; *khs = dr.hs_layer; }                 // no factor yet: the consumer writes zeros
    if constexpr (EIG) *eu = EUnit{1.0f, -1, 0.0f, 0.0f, 0.0f};       // nothing yet: zero rows, zero integrals
    float wat_a = 0.0f, wat_r = 0.0f;                                 // (KERN) the water layer's own share
    if (wet) {                                                        // surfa.f:879-910
        const float d1 = top.d;
        const float xl1 = top.rho * (top.a * top.a - 2.0f * top.b * top.b);
        const float ra = c / top.a;
        const float cr1 = ra * ra - 1.0f;
        const float mag = wvno * sqrtf(fabsf(cr1));
        if (mag <= 1.0e-35f) {
            acc.i0 = top.rho * d1;
        } else {
            float sin2ra, cosra, rab1, sinra_over;
            if (cr1 >= 0.0f) {
                sin2ra = sinf(2.0f * mag * d1) / (4.0f * mag);
                cosra = cosf(mag * d1);
                rab1 = mag * mag;
                sinra_over = sinf(mag * d1) / mag;
            } else {
                sin2ra = sinhf(2.0f * mag * d1) / (4.0f * mag);
                cosra = coshf(mag * d1);
                rab1 = -(mag * mag);
                sinra_over = sinhf(mag * d1) / mag;
            }
            const float cos2rm = 1.0f / (cosra * cosra);
            const float fac1 = (0.5f * d1 + sin2ra) * cos2rm;
            const float fac3 = wvno * (0.5f * d1 - sin2ra) * cos2rm;
            const float fac2 = wvno * fac3 / rab1;
            acc.i0 = top.rho * (fac1 + fac2);
            acc.i1 = xl1 * fac2;
            acc.i2 = xl1 * fac3;
            tzz = -top.rho * omegsq * sinra_over / cosra;
            if (KERN && !ko.raw) {
                // the water layer's own partials (the reference skips liquid layers, surfa.f:1088): in a
                // fluid the dilatation is tau_zz/lambda, so int theta^2 dz = k^2 (c/a)^4 int ur^2 dz
                const LayerRaw wraw = layer_load(mdl, fs, (size_t)b);
                const Chain ch = chain_of(wraw, lnT, false, false);
                const float dldl = -wvnosq * (ra * ra) * (ra * ra) * fac2;
                const float dldr = omegsq * (fac1 + fac2);
                wat_a = 2.0f * top.rho * top.a * cw * dldl * ch.dada;
                wat_r = cw * (dldr + top.a * top.a * dldl) * ch.rfac;
            }
        }
        if (KERN) ko.put(0, 0.0f, wat_a, wat_r);                      // (the sweep skips liquid layers)
    }
    // half-space start vectors, surfa.f:913-926, 986-989
    const LayerV hsv = layer_at(mdl, fs, (size_t)dr.hs_layer * B + b, lnT, dr.hs_layer == n - 1);
    const float cova = c / hsv.a, covb = c / hsv.b;
    const float gam = 2.0f / (covb * covb);
    const float gamm1 = gam - 1.0f;
    const float ra = wvno * sqrtf(fabsf(cova * cova - 1.0f));
    const float rb = wvno * sqrtf(fabsf(covb * covb - 1.0f));
    const float det = wvnosq - ra * rb;
    const float h = hsv.rho * omegsq;
    const float brkt = -gamm1 * wvno + gam * ra * rb / wvno;
    const double y0[4] = {1.0, 0.0, (double)(-h * brkt / det), (double)(-h * ra / det)};   // ur,uz,tz,tr
    double z0[4] = {0.0, 1.0, (double)(-h * rb / det), (double)(-h * brkt / det)};
    double y[4], z[4];
    double xnorm = 0.0, bbn = 1.0;
    // Surface fit (surfa.f:1056-1069) + one refinement (restart solution 2 from the combined start
    // vector, surfa.f:990-998).  STEP = 0: closed-form P^(4 nreg) per layer, and the restart by linearity instead of a
    // second sweep; STEP = 1: step by step, restart re-integrated (bit-consistent with the robust path's MODE 2 sweep).
    bool shorter = false;                                             // (the fast fit left the reference's split somewhere)
    auto fit = [&](auto step_tag, bool own) -> double {
        constexpr int STEP = decltype(step_tag)::value;
        for (int i = 0; i < 4; ++i) { y[i] = y0[i]; z[i] = z0[i]; }
        rayleigh_sweep<STEP, false, false, STASH>(mdl, fs, B, b, n, lnT, ndiv, water, div, dr, wvno, wvnosq, omegsq,
                             y, z, true, own, 0.0, 1.0, acc, KOut{nullptr, 1, 0, 0, 0}, 0.0f, nullptr, &shorter,
                             EOut{nullptr, 1, 0}, st);
        const double yt0 = y[0], yt1 = y[1];
        double aa = z[0] - ratio * z[1];
        double bb = ratio * yt1 - yt0;
        if (fabs(bb) < 1.e-10) bb = copysign(1.e-10, bb);
        xnorm = aa / bb;
        bb = xnorm * yt1 + z[1];
        if (fabs(bb) < 1.e-10) bb = copysign(1.e-10, bb);
        bbn = bb;
        const float ampur = (float)((xnorm * yt0 + z[0]) / bb);
        const float xtest = fabsf(ampur / ratio - 1.0f);
#if defined(SD_COUNT_RESTARTS) && defined(__HIP_DEVICE_COMPILE__)
        if (STEP == 0) {                                              // development count: restarting lanes, wavefronts
            const unsigned long long m = __ballot(xtest >= 0.00001f);
            if (m && (__lane_id() == __ffsll(__ballot(1)) - 1)) atomicAdd(&sd_restart_count[1], 1ull);
            if (xtest >= 0.00001f) atomicAdd(&sd_restart_count[0], 1ull);
        }
#endif
        if (xtest >= 0.00001f) {
            for (int i = 0; i < 4; ++i) z0[i] = z0[i] + xnorm * y0[i];
            if (STEP == 0) {
                // the RK4 map is linear: re-integrating z0 + xnorm y0 gives z + xnorm y at the surface
                for (int i = 0; i < 4; ++i) z[i] = z[i] + xnorm * y[i];
            } else {
                for (int i = 0; i < 4; ++i) z[i] = z0[i];
                rayleigh_sweep<STEP, false, false, STASH>(mdl, fs, B, b, n, lnT, ndiv, water, div, dr, wvno, wvnosq, omegsq,
                                     y, z, false, false, 0.0, 1.0, acc, KOut{nullptr, 1, 0, 0, 0}, 0.0f, nullptr, nullptr,
                                     EOut{nullptr, 1, 0}, st);
            }
            aa = z[0] - ratio * z[1];
            bb = ratio * yt1 - yt0;
            if (fabs(bb) < 1.e-10) bb = copysign(1.e-10, bb);
            xnorm = aa / bb;
            bb = xnorm * yt1 + z[1];
            if (fabs(bb) < 1.e-10) bb = copysign(1.e-10, bb);
            bbn = bb;
        }
        // growth of the fastest solution relative to the normalisation: rounding noise injected at
        // the bottom of a direct integration of the combined solution reaches eps * this at the top
        return fmax(fmax(fabs(yt0), fabs(yt1)), fmax(fabs(z[0]), fabs(z[1]))) / fabs(bbn);
    };
    const double z0_orig[4] = {z0[0], z0[1], z0[2], z0[3]};
    // The fast path's fit and sweep step its own split (fast_sublayers) together: the combined start vector is fitted
    // with the propagator that then integrates it.  Its split differs from the reference's by the RK4 error of the
    // growth factors, and the fit's cancellation amplifies that difference (measured on high-contrast stacks: U within
    // 7e-7 of the reference's split up to cancel 1e6, 2e-4 between 1e6 and 1e7): above SD_GROUP_OWN_CANCEL the fit is
    // redone in the reference's split, which the sweep then steps too (unless no layer left it: the same fit).
    bool own = SD_GROUP_LAMH > 0.0f;
    double cancel;
    for (;;) {
        cancel = fit(std::integral_constant<int, 0>{}, own);
        if (!own || !shorter || !(cancel > SD_GROUP_OWN_CANCEL) || cancel > 1.0e7) break;
        own = false;
        for (int i = 0; i < 4; ++i) z0[i] = z0_orig[i];
    }
    if (dbg) { for (int i = 0; i < 4; ++i) { dbg[i] = y[i]; dbg[4 + i] = z[i]; } dbg[12] = dr.hs_layer; dbg[13] = dr.nreg_hs; dbg[14] = ndiv; dbg[8] = xnorm; dbg[9] = bbn; }
    // half-space analytic terms use the combined vector at the top of the half space
    float aur, auz;
    const bool any_solid = (dr.hs_layer > (wet ? 1 : 0)) || (dr.nreg_hs > 0);
    (void)tzz;
    if (cancel <= 1.0e7) {
        // Fast path.  Integrate the COMBINED solution w = (xnorm*y + z)/bb itself (one 4-vector): the
        // RK4 map is linear, so this equals combining separately integrated y and z up to the
        // rounding noise the fastest-growing solution picks up on the way (<= 1e7 * 1e-16).
        for (int i = 0; i < 4; ++i) { z[i] = (xnorm * y0[i] + z0[i]) / bbn; y[i] = 0.0; }
        aur = (float)z[0]; auz = (float)z[1];
        // (EIG) the top of the effective half space is the start vector itself: the reference's entry mmax (surfa.f:1145-1148)
        if constexpr (EIG) if (dr.nreg_hs <= 0) eo.put(dr.hs_layer, aur, auz, (float)z[2], (float)z[3]);
        rayleigh_sweep<2, KERN, EIG, STASH>(mdl, fs, B, b, n, lnT, ndiv, water, div, dr, wvno, wvnosq, omegsq,
                                     y, z, false, own, xnorm, bbn, acc, ko, cw, &hold, nullptr, eo, st);
    } else {
        // Robust path (thick structure / short period: the solutions grow by up to ~1e27 and the
        // rounding noise excited on the way up is far larger than the answer).  The reference stays
        // accurate here because it combines the SAME stored knot values its fit was made with, so
        // the excited noise cancels exactly.  Do the same without storing: redo the fit step by
        // step, then step y and z again with bit-identical arithmetic (make_prop / prop_apply are
        // built with contraction off and explicit fma) and combine at every knot.
        for (int i = 0; i < 4; ++i) z0[i] = z0_orig[i];
        (void)fit(std::integral_constant<int, 1>{}, false);
        for (int i = 0; i < 4; ++i) { y[i] = y0[i]; z[i] = z0[i]; }
        aur = (float)((xnorm * y0[0] + z0[0]) / bbn);
        auz = (float)((xnorm * y0[1] + z0[1]) / bbn);
        if constexpr (EIG)
            if (dr.nreg_hs <= 0)
                eo.put(dr.hs_layer, aur, auz, (float)((xnorm * y0[2] + z0[2]) / bbn), (float)((xnorm * y0[3] + z0[3]) / bbn));
        rayleigh_sweep<2, KERN, EIG, STASH>(mdl, fs, B, b, n, lnT, ndiv, water, div, dr, wvno, wvnosq, omegsq,
                                     y, z, true, false, xnorm, bbn, acc, ko, cw, &hold, nullptr, eo, st);
    }
    if (wet && !any_solid) { aur = ratio; auz = 1.0f; }              // label 77777, surfa.f:1140-1144
    {   // label 7002, surfa.f:1145-1186
        const float xmu = hsv.rho * hsv.b * hsv.b;
        const float xlamb = hsv.rho * (hsv.a * hsv.a - 2.0f * hsv.b * hsv.b);
        const float ap = -hsv.rho * (wvno * aur + rb * auz) / det;
        const float bp = -hsv.rho * (-ra * aur / wvno - auz) / det;
        const float a1 = -wvno * ap / hsv.rho;
        const float a2 = -wvno * rb * bp / hsv.rho;
        const float a3 = ra * ap / hsv.rho;
        const float a4 = wvnosq * bp / hsv.rho;
        if (rb == 0.0f) return hsv.b;                                 // label 7006
        const double dmmr = a1 * a1 / (2.0f * ra) + 2.0f * a1 * a2 / (ra + rb) + a2 * a2 / (2.0f * rb);
        const double dmmz = a3 * a3 / (2.0f * ra) + 2.0f * a3 * a4 / (ra + rb) + a4 * a4 / (2.0f * rb);
        const double drsz = -a1 * a3 / 2.0f - (a1 * a4 * rb + a2 * a3 * ra) / (ra + rb) - a2 * a4 / 2.0f;
        const double dzsr = -a1 * a3 / 2.0f - (a1 * a4 * ra + a2 * a3 * rb) / (ra + rb) - a2 * a4 / 2.0f;
        acc.i0 += hsv.rho * (dmmr + dmmz);
        acc.i1 += (xlamb + 2.0f * xmu) * dmmr + xmu * dmmz;
        acc.i2 += xmu * dzsr - xlamb * drsz;
        if (KERN) {                                                   // surfa.f:1163-1164, 1178-1184
            const float smmz = ra * a3 * a3 / 2.0f + 2.0f * ra * rb * a3 * a4 / (ra + rb) + rb * a4 * a4 / 2.0f;
            const float smmr = ra * a1 * a1 / 2.0f + 2.0f * ra * rb * a1 * a2 / (ra + rb) + rb * a2 * a2 / 2.0f;
            const LayerRaw hraw = layer_load(mdl, fs, (size_t)dr.hs_layer * B + b);
            const K3 sh = kern_layer_rayleigh(kern_coef(hraw, hsv, lnT, dr.hs_layer == n - 1, cw, ko.raw != 0), hsv.rho, xlamb, xmu,
                                              wvno, wvnosq, omegsq, (KR)dmmr, (KR)dmmz, (KR)drsz, (KR)dzsr, (KR)smmz, (KR)smmr);
            ko.put(dr.hs_layer, hold.b + sh.b, hold.a + sh.a, hold.r + sh.r);
        }
    }
    if (dbg) { dbg[10] = acc.i0; dbg[11] = acc.i1; dbg[15] = acc.i2; }
    const float s0 = (float)acc.i0, s1 = (float)acc.i1, s2 = (float)acc.i2;
    if (KERN) *kscale = 1.0f / (-2.0f * (wvno * s1 + s2));           // 1 / (dL/dk), surfa.f:1203-1207: applied by the consumer
    if constexpr (EIG) {
        // The surface entry is SET, not integrated: (ratio, 1, 0, 0) (surfa.f:1231-1245).  Under a water layer the
        // reference's first entry is the sea floor, dept1(1) = d(1), with the water's normal traction: (ratio, 1, tzz, 0)
        // (surfa.f:1232, 1244) - caller layer 1; the sea surface itself, which the reference does not form, is zero.
        if (wet) {
            eo.put(0, 0.0f, 0.0f, 0.0f, 0.0f);
            if (dr.hs_layer >= 1) eo.put(1, ratio, 1.0f, tzz, 0.0f);
        } else {
            eo.put(0, ratio, 1.0f, 0.0f, 0.0f);
        }
        *eu = EUnit{1.0f, dr.hs_layer, s0, s1, s2};
    }
    return (wvno * s1 + s2) / (omega * s0);                           // surfa.f:1186
}

// ---- Love, surfa.f:374-606 (all fp32, as the reference) --------------------------------------
template <bool KERN = false, bool EIG = false>
SD_HD float group_love(const float *__restrict__ mdl, size_t fs, int B, int b, int n,
                            float T, float c, const KOut ko = KOut{nullptr, 1, 0, 0, 0}, float *kscale = nullptr, int *khs = nullptr,
                            const EOut eo = EOut{nullptr, 1, 0}, EUnit *eu = nullptr)
{
    const float lnT = logf(1.0f / T);
    int ndiv = 5;
    const int ivre = 999 / (n - 1);                                   // surfa.f:414-415
    if (ndiv > ivre) ndiv = ivre;
    if (ndiv < 1) ndiv = 1;
    const float div = (float)ndiv;
    const LayerV top = layer_at(mdl, fs, (size_t)b, lnT, false);
    const bool water = (ndiv > 1) ? (top.b <= 0.1e-10f) : false;
    const Drop dr = drop_or_none<1>(mdl, fs, B, b, n, lnT, c, T, ndiv, water, div);
    const float wvno = 6.2831853f / (c * T);
    const LayerV hsv = layer_at(mdl, fs, (size_t)dr.hs_layer * B + b, lnT, dr.hs_layer == n - 1);
    constexpr bool kern = KERN;
    const float wvnosq = wvno * wvno;
    const float omega = 6.2831853f / T, omegsq = omega * omega;
    const float cw = c / wvno;
    // one layer's share of dc/db, dc/drho (surfa.f:509-512, 561-565), still to be divided by dL/dk
    auto kern_layer = [&](int jl, const LayerRaw &raw, const LayerV &v, float dm, float sm) -> K3 {
        const Chain ch = chain_of(raw, lnT, jl == n - 1, ko.raw != 0);
        const float dldm = -(wvnosq * dm + sm);
        const float dldr = omegsq * dm;
        return K3{2.0f * v.rho * v.b * cw * dldm * ch.dbdb, 0.0f, cw * (dldr + v.b * v.b * dldm) * ch.rfac};
    };
    if (kern) { *kscale = 0.0f; *khs = dr.hs_layer; }
    if constexpr (EIG) *eu = EUnit{1.0f, -1, 0.0f, 0.0f, 0.0f};       // nothing yet (attempts exhausted: zero rows, zero integrals)
    float ut0 = 1.0f;
    for (int attempt = 0; attempt < 16; ++attempt) {
        float ut = ut0;
        K3 hold{0.0f, 0.0f, 0.0f};                                    // (KERN) share of the layer that holds the half space
        const float covb = c / hsv.b;
        const float hh = hsv.rho * hsv.b * hsv.b;
        const float rbh = wvno * sqrtf(fabsf(covb * covb - 1.0f));
        float tq = -hh * rbh * ut0;
        const float dm0 = (rbh == 0.0f) ? 1.0e25f : 0.5f / rbh;
        float sumi0 = hsv.rho * dm0;
        float sumi1 = hh * dm0;
        bool overflow = false;
        LayerRaw nraw = layer_load(mdl, fs, (size_t)dr.hs_layer * B + b);
        // the half space itself (surfa.f:502-512): int u^2 = 1/(2 rb), int (du/dz)^2 = rb/2 - like the reference's sumi0 /
        // sumi1 start values not scaled with ut0^2
        if (kern && rbh > 0.0f) hold = kern_layer(dr.hs_layer, nraw, hsv, dm0, 0.5f * rbh);
        // (EIG) the top of the effective half space: amp(mmax), stress(mmax) (surfa.f:499-500).  A retry after an overflow
        // (ut0 / 1e5) rewrites every store of the failed attempt.
        if constexpr (EIG) if (dr.nreg_hs <= 0) eo.put2(dr.hs_layer, ut, tq);
        for (int jl = dr.hs_layer; jl >= 0 && !overflow; --jl) {
            const LayerRaw raw = nraw;
            if (jl > 0) nraw = layer_load(mdl, fs, (size_t)(jl - 1) * B + b);
            const int nsub = (jl == 0 && water) ? 1 : ndiv;
            const int nreg = (jl == dr.hs_layer) ? dr.nreg_hs : nsub;
            if (nreg <= 0) continue;
            const LayerV v = layer_derive(raw, lnT, jl == n - 1);
            if (v.b == 0.0f) {                                        // surfa.f:524 (still tests |ut|)
                if (fabsf(ut) > 1.0e10f) overflow = true;
                if (kern && jl != dr.hs_layer) ko.put(jl, 0.0f, 0.0f, 0.0f);
                continue;
            }
            const float dsub = (ndiv > 1 && !(jl == 0 && water)) ? v.d / div : v.d;
            const float cv = c / v.b;
            const float rb = wvno * sqrtf(fabsf(cv * cv - 1.0f));
            const float h = v.rho * v.b * v.b;
            const float dz = dsub / 4.0f;
            // the four quarter-step propagators are the same for every sublayer of this layer
            float yk[4], zk[4], ck[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const float xkk = (float)(kk + 1);
                const float q = rb * dz * xkk;
                if (c < v.b) {
                    const float ep = expf(q), emq = 1.0f / ep;
                    yk[kk] = (ep - emq) / (2.0f * rb);
                    zk[kk] = rb * rb * yk[kk];
                    ck[kk] = (ep + emq) / 2.0f;
                } else if (c == v.b) {
                    yk[kk] = dz * xkk; zk[kk] = 0.0f; ck[kk] = 1.0f;
                } else {
                    float sn, cs; sincosf(q, &sn, &cs);
                    yk[kk] = sn / rb; zk[kk] = -rb * sn; ck[kk] = cs;
                }
            }
            float k_dm = 0.0f, k_sm = 0.0f;
            for (int s = 0; s < nreg; ++s) {
                if (fabsf(ut) > 1.0e10f) { overflow = true; break; } // surfa.f:519-522
                float dmm[5], smm[5];
                dmm[0] = ut * ut;
                if (kern) smm[0] = (tq / h) * (tq / h);
                float eut = ut, ett = tq;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    eut = ck[kk] * ut - yk[kk] * tq / h;
                    ett = -h * zk[kk] * ut + ck[kk] * tq;
                    dmm[kk + 1] = eut * eut;
                    if (kern) smm[kk + 1] = (ett * ett) / (h * h);
                }
                ut = eut; tq = ett;
                const float dm = (dz / 22.5f) * (7.0f * (dmm[0] + dmm[4]) + 32.0f * (dmm[1] + dmm[3]) + 12.0f * dmm[2]);
                sumi0 = sumi0 + v.rho * dm;
                sumi1 = sumi1 + h * dm;
                if (kern) {
                    k_dm += dm;
                    k_sm += (dz / 22.5f) * (7.0f * (smm[0] + smm[4]) + 32.0f * (smm[1] + smm[3]) + 12.0f * smm[2]);
                }
            }
            if constexpr (EIG) if (!overflow) eo.put2(jl, ut, tq);   // after the layer's last sublayer: its top
            if (kern && !overflow) {
                const K3 sh = kern_layer(jl, raw, v, k_dm, k_sm);
                if (jl == dr.hs_layer) { hold.b += sh.b; hold.r += sh.r; }
                else ko.put(jl, sh.b, 0.0f, sh.r);
            }
        }
        if (overflow) { ut0 = ut0 / 1.0e5f; continue; }
        if (kern) {                                                   // surfa.f:581-585
            ko.put(dr.hs_layer, hold.b, 0.0f, hold.r);
            *kscale = 1.0f / (-2.0f * wvno * sumi1);                  // 1 / (dL/dk): applied by the consumer
        }
        sumi0 = sumi0 / (ut * ut);
        sumi1 = sumi1 / (ut * ut);
        if constexpr (EIG) {
            // The surface entry is SET: (1, 0) (surfa.f:627-628) - stored as (ut, 0), which the consumer's division by ut
            // makes exactly (1, 0).  Under a water layer, which LEIGEN skips (surfa.f:524, 579), ut is the value at the sea
            // floor, the reference's first entry (dept1(1) = d(1), surfa.f:626): caller layer 1; the sea surface is zero.
            if (!(top.b > 0.0f)) {
                eo.put2(0, 0.0f, 0.0f);
                if (dr.hs_layer >= 1) eo.put2(1, ut, 0.0f);
            } else {
                eo.put2(0, ut, 0.0f);
            }
            if (ut != 0.0f && fin(ut)) *eu = EUnit{ut, dr.hs_layer, sumi0, sumi1, 0.0f};
        }
        return sumi1 / (c * sumi0);                                   // surfa.f:606
    }
    return 0.0f;
}

// KERN: also write the analytic partials (A.kb/ka/kr).  The plain variant is held to 168 VGPRs (three
// wavefronts per SIMD instead of two).  EIG: also store the eigenfunction at every layer top and the energy integrals (K2d).
// STASH (surfdisp_group_kernel_stash, the default Rayleigh launch of a shallow batch: launch_group): gstash is the
// workgroup's dynamic LDS, [Lmax][SD_STASH_W][256] - the lanes' layer values from the fit for the later sweeps (LStash).
#ifndef SD_GROUP_WAVES
#define SD_GROUP_WAVES 3
#endif
#ifndef SD_KERN_WAVES
#define SD_KERN_WAVES 1
#endif
template <int KIND, bool KERN, bool EIG, bool STASH>
__device__ __forceinline__ void group_kernel_body(const GroupArgs &A, float *gstash)
{
    const int B = A.B, P = A.P;
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    int b, k;                                               // a wavefront = 64 stacks, one period
    if (A.xcd_order) {
        // Workgroups go to the 8 XCDs in turn (blockIdx % 8), each with its own L2.  In plain period-major order the P
        // workgroups that read the same 256 stacks are B/256 launches apart and every one of them fetches the stacks from HBM
        // again, once per sweep (16 384 x L64 x P20: 0.5 .. 0.8 GB per launch for 17 MB of stacks).  Here XCD x takes the stack
        // blocks x, x + 8, ... g at a time, period by period: the P readers of a stack block run on one XCD, close in time.
        const int g = A.xcd_order;                          // stack blocks an XCD works on at a time, period by period
        const int x = blockIdx.x & 7, q = blockIdx.x >> 3;
        const int r = q % (g * P);
        k = r / g;
        b = (((q / (g * P)) * g + r % g) * 8 + x) * 256 + (int)threadIdx.x;
        if (b >= B) return;
        if (A.krev) k = P - 1 - k;
        idx = (size_t)k * B + b;
    } else {
        if (idx >= (size_t)B * P) return;
        b = (int)(idx % B); k = (int)(idx / B);
        if (A.krev) { k = P - 1 - k; idx = (size_t)k * B + b; }
    }
    const size_t o = idx;                                   // period-major [P][B]: coalesced
    const int n = A.nl[b];
    KOut ko{nullptr, 1, 0, 0, 0};
    float *ra_ = nullptr, *rr_ = nullptr;                   // direct route: this unit's dc/dVp, dc/drho rows
    if (KERN) {
        ko.raw = A.kraw;
        if (A.kscr) {                                       // layer-major scratch [3][Lmax][P][B]: coalesced
            const size_t arr = (size_t)A.Lmax * P * B;
            ko.stride = (size_t)P * B;
            ko.b = A.kscr + idx;
            ko.off_a = (KIND == 2 && A.ka) ? (ptrdiff_t)(arr * sizeof(float)) : 0;
            ko.off_r = A.kr ? (ptrdiff_t)(2 * arr * sizeof(float)) : 0;
        } else {                                            // the caller's [B][P][Lmax] rows (small workspace)
            const size_t ro = ((size_t)b * P + k) * A.Lmax;
            ko.stride = 1;
            ko.b = A.kb + ro;
            ra_ = A.ka ? A.ka + ro : nullptr;
            rr_ = A.kr ? A.kr + ro : nullptr;
            // (uniform byte distances between the caller's arrays; Love has no dc/dVp: its rows are zero-filled below)
            ko.off_a = (KIND == 2 && A.ka) ? (ptrdiff_t)(reinterpret_cast<const char *>(A.ka) - reinterpret_cast<const char *>(A.kb)) : 0;
            ko.off_r = A.kr ? (ptrdiff_t)(reinterpret_cast<const char *>(A.kr) - reinterpret_cast<const char *>(A.kb)) : 0;
        }
    }
    float kscale = 0.0f;
    int khs = -1;
    float ugr = 0.0f;
    EOut eo{nullptr, 1, 0};
    EUnit eu{1.0f, -1, 0.0f, 0.0f, 0.0f};
    if constexpr (EIG) {                                    // layer-major scratch [4][Lmax][P][B]: coalesced
        eo.p = A.escr + idx;
        eo.stride = (size_t)P * B;
        eo.plane = (size_t)A.Lmax * P * B;
    }
    if (n >= 2 && k < A.nsolved[b]) {
        const size_t fs = (size_t)A.Lmax * B;
        const float T = A.per[k];
        const float c = A.c[o];
                if (KIND == 2 && STASH) {    // (launch_group: the default Rayleigh launch of a shallow batch)
            LStash st{gstash + threadIdx.x, 256};
            ugr = group_rayleigh<false, false, true>(A.mdl, fs, B, b, n, T, c, A.ratio[(size_t)k * B + b],
                                               A.dbg ? A.dbg + 16 * o : nullptr, ko, &kscale, &khs, eo, &eu, &st);
        } else if (KIND == 2) ugr = group_rayleigh<KERN, EIG>(A.mdl, fs, B, b, n, T, c, A.ratio[(size_t)k * B + b],
                                                       A.dbg ? A.dbg + 16 * o : nullptr, ko, &kscale, &khs, eo, &eu);
        else           ugr = group_love<KERN, EIG>(A.mdl, fs, B, b, n, T, c, ko, &kscale, &khs, eo, &eu);
    }
    if constexpr (EIG) {
        // (no finite integrals: zeros, as for an unsolved unit)
        if (!(fabsf(eu.i0) <= 3.0e38f) || !(fabsf(eu.i1) <= 3.0e38f) || !(fabsf(eu.i2) <= 3.0e38f)) eu = EUnit{1.0f, -1, 0.0f, 0.0f, 0.0f};
        const size_t PB = (size_t)P * B;
        A.ediv[o] = eu.div; A.ehs[o] = eu.hs;
        A.esum[o] = eu.i0; A.esum[PB + o] = eu.i1; A.esum[2 * PB + o] = eu.i2;
    }
    if (KERN) {
        if (!(fabsf(kscale) <= 3.0e38f)) kscale = 0.0f;     // (no finite factor: zeros, as for an unsolved unit)
        if (A.kscr) { A.kscale[o] = kscale; A.khs[o] = (kscale != 0.0f) ? khs : -1; }
        else {
            // direct route: the lane finishes its own rows - the products the transposition kernel forms on the scratch route
            const int top = (kscale != 0.0f) ? khs : -1;
            for (int i = 0; i < A.Lmax; ++i) {
                ko.b[i] = (i <= top) ? ko.b[i] * kscale : 0.0f;
                if (ra_) ra_[i] = (KIND == 2 && i <= top) ? ra_[i] * kscale : 0.0f;
                if (rr_) rr_[i] = (i <= top) ? rr_[i] * kscale : 0.0f;
            }
        }
    }
    A.u[o] = ugr;
}
template <int KIND, bool KERN, bool EIG = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KERN ? SD_KERN_WAVES : SD_GROUP_WAVES, 8)))
void surfdisp_group_kernel(GroupArgs A)
{
    group_kernel_body<KIND, KERN, EIG, false>(A, nullptr);
}
// the plain Rayleigh kernel, KIND = 2, with the layer stash (a kernel of its own: with both paths in one kernel the
// register allocation of either spills at the 168 VGPRs that three wavefronts per SIMD allow)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SD_GROUP_WAVES, 8)))
void surfdisp_group_kernel_stash(GroupArgs A)
{
    extern __shared__ float gstash[];
    group_kernel_body<2, false, false, true>(A, gstash);
}

// K3: period-major internal results -> the caller's [B][P] arrays, through an LDS tile so that both
// the reads (along b) and the writes (whole rows of consecutive stacks) are coalesced.
__global__ __launch_bounds__(256) void surfdisp_finish_kernel(FinishArgs A)
{
    extern __shared__ float tile[];                 // [64][P+1]
    const int B = A.B, P = A.P, PS = P + 1;
    const int b0 = blockIdx.x * 64;
    const int nb = min(64, B - b0);
    if (A.nsolved && threadIdx.x < nb) {
        // independent mode: status word from the reduced first-failing period
        const int bb = b0 + threadIdx.x;
        const int ns = A.nsolved[bb];
        if (A.status) A.status[bb] = (A.nl[bb] < 2) ? SURFDISP_BADMODEL
                                     : (ns >= P ? SURFDISP_OK
                                     : (ns < 0 ? SURFDISP_NUMERIC : (ns == 0 ? SURFDISP_NOROOT : SURFDISP_PARTIAL)));
    }
    for (int pass = 0; pass < 3; ++pass) {
        const float *src = (pass == 0) ? A.ct : (pass == 1 ? A.ut : A.rt);
        float *dst = (pass == 0) ? A.c : (pass == 1 ? A.u : A.ratio);
        if (!src || !dst) continue;                 // phase-only call: no group velocities (block-uniform)
        for (int i = threadIdx.x; i < 64 * P; i += 256) {
            const int k = i / 64, bl = i % 64;
            if (bl < nb) {
                float v = src[(size_t)k * B + b0 + bl];
                if (A.nsolved && k >= A.nsolved[b0 + bl]) v = 0.0f;   // independent mode: failure cascade
                // the ellipticity slot of an unsolved period was never written
                if (pass == 2 && (k >= A.nsolved_all[b0 + bl] || A.nl[b0 + bl] < 2)) v = 0.0f;
                tile[bl * PS + k] = v;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < nb * P; i += 256) {
            const int bl = i / P, k = i % P;
            dst[(size_t)b0 * P + i] = tile[bl * PS + k];
        }
        __syncthreads();
    }
}

// K2b: the analytic partials from the layer-major scratch [3][Lmax][P*B] to the caller's [B][P][Lmax] rows
// (rows_through_tile, surfdisp_k_rows.h).  Applies the unit's factor 1 / (dL/dk) and writes zeros below the unit's deepest
// layer (entries the group-velocity kernel never wrote are not read).  blockIdx.z: 0 dc/dVs, 1 dc/dVp, 2 dc/drho.
__global__ __launch_bounds__(256) void surfdisp_kern_transpose_kernel(KernTransposeArgs A)
{
    const int B = A.B, P = A.P, Lmax = A.Lmax;
    float *__restrict__ out = (blockIdx.z == 0) ? A.kb : ((blockIdx.z == 1) ? A.ka : A.kr);
    if (!out) return;                                        // (block-uniform)
    const size_t PB = (size_t)P * B;
    const float *__restrict__ scr = A.kscr + (size_t)blockIdx.z * Lmax * PB;
    const bool zero_only = (blockIdx.z == 1) && (A.kind != 2);   // Love has no dc/dVp
    const RowTile t = row_tile(B);
    float sc = 0.0f; int hs = -1;
    if (t.live && !zero_only) { sc = A.kscale[t.un]; hs = A.khs[t.un]; }
    rows_through_tile(t, B, P, Lmax, out, [&](int i) { return (i <= hs) ? scr[(size_t)i * PB + t.un] * sc : 0.0f; });
}

// K2d: the eigenfunctions (surfdisp_forward_eigen_device) from the layer-major scratch [4][Lmax][P*B] the EIG group-velocity
// kernel leaves (EOut / EUnit) to the caller's [B][P][Lmax] rows (rows_through_tile, surfdisp_k_rows.h).  Divides by the
// unit's divisor as the reference does (amp(l) / ut, surfa.f:580-581; Rayleigh: 1), writes zeros below the unit's deepest
// layer and for units without one (unsolved periods, bad stacks, degenerate exits), and whole rows.  blockIdx.z: 0 ur (Love:
// the transverse displacement), 1 uz, 2 tz, 3 tr (Love: the shear traction); Love's uz and tz are rows of zeros.
// Love's low-amplitude exclusion (surfa.f:588-596): an entry whose layer is at least as fast as the effective half space and
// whose normalised displacement is below xxmin = 1e-20 is zero, displacement and traction.
// energy [B][P][4] = (I0, I1, I2, amp), amp = 1 / (2 c U I0) rounded once to fp32, 0 where c is not a solved value: the
// surface-wave amplification factor.  The reference's amplitude response (surfa.f:608, 1191) is are = ale = amp x
// 1e-15 / sqrt(6.28318): a constant factor away.
__global__ __launch_bounds__(256) void surfdisp_eigen_transpose_kernel(EigenTransposeArgs A)
{
    const int B = A.B, P = A.P, Lmax = A.Lmax;
    const int z = blockIdx.z;
    float *__restrict__ out = (z == 0) ? A.ur : ((z == 1) ? A.uz : ((z == 2) ? A.tz : A.tr));
    if (!out) return;                                        // (block-uniform)
    const bool love = A.kind != 2;
    const bool zero_only = love && (z == 1 || z == 2);
    const size_t PB = (size_t)P * B;
    const float *__restrict__ scr = A.escr + (size_t)(love ? (z == 3 ? 1 : 0) : z) * Lmax * PB;
    const RowTile t = row_tile(B);
    const int k = t.k, b = t.b0 + t.bl;
    const bool live = t.live;
    const size_t un = t.un;
    float dv = 1.0f; int hs = -1;
    if (live && !zero_only) { dv = A.ediv[un]; hs = A.ehs[un]; }
    if (z == 0 && blockIdx.y == 0 && A.energy && threadIdx.x < 64 && live) {
        float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f, amp = 0.0f;
        if (hs >= 0) {
            e0 = A.esum[un]; e1 = A.esum[PB + un]; e2 = A.esum[2 * PB + un];
            const float c = A.c[un], u = A.u[un];
            if (c > 0.0f) amp = (float)(1.0 / (2.0 * (double)c * (double)u * (double)e0));
            if (!fin(amp)) amp = 0.0f;
        }
        float *e = A.energy + ((size_t)b * P + k) * 4;
        e[0] = e0; e[1] = e1; e[2] = e2; e[3] = amp;
    }
    rows_through_tile(t, B, P, Lmax, out, [&](int i) {
        float v = 0.0f;
        if (i <= hs) {
            v = scr[(size_t)i * PB + un] / dv;
            if (love) {
                const float amp = (z == 0) ? v : A.escr[(size_t)i * PB + un] / dv;
                if (fabsf(amp) < 1.0e-20f) {                 // (rare: only then are the two velocities formed)
                    const float lnT = logf(1.0f / A.per[k]);
                    const size_t fs = (size_t)Lmax * B;
                    const int n = A.nl[b];
                    const float vb = layer_at(A.mdl, fs, (size_t)i * B + b, lnT, i == n - 1).b;
                    const float vh = layer_at(A.mdl, fs, (size_t)hs * B + b, lnT, hs == n - 1).b;
                    if (vb >= vh) v = 0.0f;
                }
            }
        }
        return v;
    });
}

// K2c: the apparent attenuation of the mode from the same scratch (surfdisp_forward_atten_device).  After REIGEN / LEIGEN the
// reference forms, from its partials and the layers' 1/Qs (calcul.f:256-265, 341-349; dwx: surfa.f:1207),
//      W_i = b_i (dc/db_i + 4/3 (b_i / a_i) dc/da_i)   (Love: b_i dc/db_i),        S = sum_i qsinv_i W_i,
//      alpha = pi S / (T c^2),     1 / Q_app = S U / c^2,
// in a loop whose bound is never assigned, into locals nothing returns.  Here W_i comes from the caller-coordinate shares
// kb = dc/dVs, ka = dc/dVp the scratch holds - scaled with the unit's factor in fp32 exactly as K2b scales them, so the
// result is a function of the rows the caller receives - by undoing the chain factors of chain_of (the flattening factor
// cancels; qsq = qsinv ln(1/T) / pi, qpq = qsq 4/3 Vs^2 / Vp^2):
//      W_i = Vs kb - Vs ka (8/3) qsq (Vs/Vp) / (1 - qpq) + (4/3) ka Vs^2 (1 + qsq)^2 / (Vp (1 + qpq) (1 - qpq)),
// in fp64 (the three terms may cancel; the kernel is bound by its reads).  dqdq_i = W_i U / c^2 is the linear kernel of
// 1 / Q_app with respect to layer i's 1/Qs at fixed eigenfunction; 1 / Q_app = sum_i dqdq_i qsinv_i.
// One workgroup = 64 consecutive stacks at one period (a wavefront reads consecutive words of every layer plane) x 4
// wavefronts that take every fourth layer; per 64-layer tile the dqdq values go through LDS to whole rows as in K2b, the
// four partial sums (fp64, fixed order) meet in LDS at the end.  Zeros: units without a factor (unsolved periods, bad
// stacks), water layers, layers below the unit's half space.
template <int KIND>
__global__ __launch_bounds__(256) void surfdisp_atten_kernel(AttenArgs A)
{
    __shared__ float tile[64][65];
    __shared__ double part[4][64];
    const int B = A.B, P = A.P, Lmax = A.Lmax;
    const int nbb = (B + 63) / 64;
    const int k = blockIdx.x / nbb, b0 = (blockIdx.x % nbb) * 64;
    const size_t PB = (size_t)P * B, fs = (size_t)Lmax * B;
    const int bl = threadIdx.x % 64, wv = threadIdx.x / 64;
    const int b = b0 + bl;
    const float *__restrict__ scr_b = A.kscr;
    const float *__restrict__ scr_a = A.kscr + (size_t)Lmax * PB;
    const float *__restrict__ mdl = A.mdl;
    float sc = 0.0f; int hs = -1;
    double uc2 = 0.0, ut = 0.0, lnT = 0.0;
    if (b < B) {
        const size_t o = (size_t)k * B + b;
        const float c = A.c[o], u = A.u[o], T = A.per[k];
        sc = A.kscale[o];
        if (sc != 0.0f && c > 0.0f && u > 0.0f) {
            hs = A.khs[o];
            uc2 = (double)u / ((double)c * (double)c);
            ut = (double)u * (double)T;
            lnT = log(1.0 / (double)T);
        }
    }
    double sum = 0.0;
    for (int i0 = 0; i0 < Lmax; i0 += 64) {
        for (int il = wv; il < 64; il += 4) {
            const int i = i0 + il;
            double dq = 0.0;
            if (i <= hs) {
                const size_t ol = (size_t)i * B + b;
                const double vs = (double)mdl[F_VS * fs + ol];
                if (vs > 0.0) {                                          // (a water layer has no share)
                    const double qs = (double)mdl[F_QS * fs + ol];
                    double w = vs * (double)(scr_b[(size_t)i * PB + (size_t)k * B + b] * sc);
                    if (KIND == 2) {
                        const double vp = (double)mdl[F_VP * fs + ol];
                        const double ka = (double)(scr_a[(size_t)i * PB + (size_t)k * B + b] * sc);
                        const double qsq = qs * lnT / 3.14159265358979323846;
                        const double qpq = qsq * (4.0 / 3.0) * vs * vs / (vp * vp);
                        w = w - vs * ka * (8.0 / 3.0) * qsq * (vs / vp) / (1.0 - qpq)
                              + (4.0 / 3.0) * ka * vs * vs * (1.0 + qsq) * (1.0 + qsq) / (vp * (1.0 + qpq) * (1.0 - qpq));
                    }
                    dq = w * uc2;
                    sum += dq * qs;
                }
            }
            if (A.dqdq) tile[il][bl] = (float)dq;
        }
        if (A.dqdq) {                                                    // (block-uniform)
            __syncthreads();
            for (int t = threadIdx.x; t < 64 * 64; t += 256) {
                const int bq = t / 64, il = t % 64;
                if (i0 + il < Lmax && b0 + bq < B) A.dqdq[((size_t)(b0 + bq) * P + k) * Lmax + i0 + il] = tile[il][bq];
            }
            __syncthreads();
        }
    }
    part[wv][bl] = sum;
    __syncthreads();
    if (wv == 0 && b < B) {
        const double q = ((part[0][bl] + part[1][bl]) + part[2][bl]) + part[3][bl];
        A.qinv[(size_t)b * P + k] = (float)q;                            // (0 for a unit without partials)
        if (A.gamma) A.gamma[(size_t)b * P + k] = (hs >= 0) ? (float)(3.14159265358979323846 * q / ut) : 0.0f;
    }
}

// K2e: the thickness and interface-depth kernels of the phase velocity (surfdisp_forward_thickness_kernels_device) from the two
// layer-major scratches: the layer-top eigenfunctions of the EIG group-velocity kernel (K2d) and the unscaled shares of
// dc/d(Vs, Vp, rho) (K2b).  With v_j the displacement-stress vector at the top of caller layer j, normalised as K2d returns it,
// (a, b, rho)_m the values layer_at gives, lam = rho (a^2 - 2 b^2), mu = rho b^2, k = omega / c, the Hamiltonian of the depth ODE
//      Love      E(v; m) = rho omega^2 ut^2 - mu k^2 ut^2 + tq^2 / mu
//      Rayleigh  uz' = (tz + k lam ur) / (lam + 2 mu), ur' = tr / mu - k uz,
//                W2 = lam (uz' - k ur)^2 + 2 mu (k^2 ur^2 + uz'^2) + mu (ur' + k uz)^2,
//                E(v; m) = rho omega^2 (ur^2 + uz^2) - W2 + 2 tr ur' + 2 tz uz'
//      liquid layer above the sea floor (lam = rho a^2): urw = -k tz / (rho omega^2), uz' = tz / lam + k urw,
//                E = rho omega^2 (urw^2 + uz^2) - tz^2 / lam + 2 tz uz'             (Love: 0, the sea floor is its free surface)
// is constant through a homogeneous layer, and its jump is the kernel of the flattened depth of interface j (1 <= j <= hs, the
// unit's effective half space), the other interfaces and omega fixed:
//      K_j = -amp (c^3 / omega^2) [E(v_j; j-1) - E(v_j; j)],      amp = 1 / (2 c U I0).
// The caller's depth of interface j also moves the flattening factors of the two layers it bounds (flat1.f:44-62; r_j = R0 -
// sum_{m<j} h_m, rt / rb a layer's top / bottom radius, x = ln(rt / rb), p = pwr_of; q^p = (rb / rt)^p = exp(-p x)):
//      d ln dif/d rt =  1 / (rt^2 (1/rb - 1/rt)) - 1 / (x rt),      d ln dif/d rb = -1 / (rb^2 (1/rb - 1/rt)) + 1 / (x rb),
//      d ln qqq/d rt =  p / (rt (1 - q^p)) - 1 / (x rt),            d ln qqq/d rb = -p q^p / (rb (1 - q^p)) + 1 / (x rb),
//      (the layer nlay - 1 in its half-space role: -1 / rt and p / rt),
// which act on c through the caller-coordinate shares Sv_m = Vs dc/dVs + Vp dc/dVp, Sr_m = rho dc/drho - the scratch values
// times the unit's factor in fp32, exactly the rows K2b writes (a' is homogeneous of degree 1 in (Vp, Vs), so Sv is the share
// of ln dif):
//      dcdz_j = K_j R0 / r_j - [Sv_{j-1} d ln dif_{j-1}/d rb + Sr_{j-1} d ln qqq_{j-1}/d rb] - [Sv_j d ln dif_j/d rt + Sr_j d ln qqq_j/d rt],
//      dcdh_i = sum_{j>i} dcdz_j       (layer i thicker, everything below shifted rigidly).
// All in fp64 (the 1/h-sized terms of the factor derivatives cancel down to 1/r).  Left out: the factor term of a liquid
// layer (its shares are not read), the dependence of the layer dropping on the thicknesses (as in every other row), and the
// share of a layer without thickness (it holds no energy).
// ThickUnit: what one (stack, period) unit needs; entry (component q, layer i) of its layer-top values sits at
// ev[q * e_plane + i * e_layer], its shares (0 Vs, 1 Vp, 2 rho) at kv[q * k_plane + i * k_layer].
struct ThickUnit {
    const float *mdl; size_t fs; int B, b, n;
    int hs;                       // deepest interface with a kernel; < 1: a unit of zeros
    int khs;                      // deepest layer with shares
    bool wet;
    float lnT, dv, ksc;
    double k, om2, fac;           // wavenumber, omega^2, -amp c^3 / omega^2
    const float *ev; size_t e_layer, e_plane;
    const float *kv; size_t k_layer, k_plane;
};
SD_HD inline ThickUnit thick_unit(const float *mdl, size_t fs, int B, int b, int n, float T, float c, float u, float i0,
                                  float dv, int ehs, float ksc, int khs, const float *ev, size_t e_layer, size_t e_plane,
                                  const float *kv, size_t k_layer, size_t k_plane)
{
    ThickUnit q;
    q.mdl = mdl; q.fs = fs; q.B = B; q.b = b; q.n = n;
    q.ev = ev; q.e_layer = e_layer; q.e_plane = e_plane; q.kv = kv; q.k_layer = k_layer; q.k_plane = k_plane;
    q.dv = dv; q.ksc = ksc; q.khs = khs;
    q.hs = (n >= 2 && ksc != 0.0f && c > 0.0f && ehs <= n - 1) ? ehs : -1;
    q.wet = false; q.lnT = 0.0f; q.k = 0.0; q.om2 = 0.0; q.fac = 0.0;
    if (q.hs >= 1) {
        const double om = (double)6.2831853072f / (double)T;
        q.lnT = logf(1.0f / T);
        q.k = om / (double)c;
        q.om2 = om * om;
        q.fac = -(1.0 / (2.0 * (double)c * (double)u * (double)i0)) * ((double)c * (double)c * (double)c) / q.om2;
        q.wet = !(mdl[F_VS * fs + (size_t)b] > 0.0f);
    }
    return q;
}
SD_HD __forceinline__ double thick_energy_love(double ut, double tq, const LayerV &v, double k, double om2)
{
#pragma clang fp contract(off)
    const double rho = v.rho, mu = rho * ((double)v.b * (double)v.b);
    return rho * om2 * (ut * ut) - mu * (k * k) * (ut * ut) + tq * tq / mu;
}
SD_HD __forceinline__ double thick_energy_rayleigh(double ur, double uz, double tz, double tr, const LayerV &v, double k, double om2)
{
#pragma clang fp contract(off)
    const double rho = v.rho, b2 = (double)v.b * (double)v.b, mu = rho * b2;
    const double lam = rho * ((double)v.a * (double)v.a - 2.0 * b2);
    const double duz = (tz + k * lam * ur) / (lam + 2.0 * mu);
    const double dur = tr / mu - k * uz;
    const double e1 = duz - k * ur, e2 = dur + k * uz;
    const double w2 = lam * (e1 * e1) + 2.0 * mu * (k * k * (ur * ur) + duz * duz) + mu * (e2 * e2);
    return rho * om2 * (ur * ur + uz * uz) - w2 + 2.0 * tr * dur + 2.0 * tz * duz;
}
SD_HD __forceinline__ double thick_energy_liquid(double uz, double tz, const LayerV &v, double k, double om2)
{
#pragma clang fp contract(off)
    const double rho = v.rho, lam = rho * ((double)v.a * (double)v.a);
    const double urw = -k * tz / (rho * om2);
    const double duz = tz / lam + k * urw;
    return rho * om2 * (urw * urw + uz * uz) - tz * tz / lam + 2.0 * tz * duz;
}
// the caller-coordinate shares (Sv, Sr) of layer m: K2b's fp32 products; a liquid layer and a layer below khs have none
template <int KIND>
SD_HD __forceinline__ void thick_shares(const ThickUnit &q, int m, double *sv, double *sr)
{
#pragma clang fp contract(off)
    *sv = 0.0; *sr = 0.0;
    if (m > q.khs) return;
    const size_t ol = (size_t)m * q.B + q.b;
    const float vs = q.mdl[F_VS * q.fs + ol];
    if (!(vs > 0.0f)) return;
    const float *p = q.kv + (size_t)m * q.k_layer;
    const float kb = p[0] * q.ksc, kr = p[2 * q.k_plane] * q.ksc;
    double s = (double)vs * (double)kb;
    if (KIND == 2) {
        const float ka = p[q.k_plane] * q.ksc;
        s = s + (double)q.mdl[F_VP * q.fs + ol] * (double)ka;
    }
    *sv = s;
    *sr = (double)q.mdl[F_RHO * q.fs + ol] * (double)kr;
}
// dcdz_j of interface j (1 <= j <= q.hs): z_up the depth of the top of layer j - 1 (the fp64 sum of the thicknesses above
// it, in layer order), h_up and h_dn the thicknesses of the layers j - 1 and j.  *kj: the flattened-depth kernel K_j.
template <int KIND>
SD_HD inline double thick_interface(const ThickUnit &q, int j, double z_up, float h_up, float h_dn, double *kj)
{
#pragma clang fp contract(off)
    const float *e = q.ev + (size_t)j * q.e_layer;
    const LayerV up = layer_at(q.mdl, q.fs, (size_t)(j - 1) * q.B + q.b, q.lnT, false);
    const LayerV dn = layer_at(q.mdl, q.fs, (size_t)j * q.B + q.b, q.lnT, j == q.n - 1);
    const bool sea_floor = q.wet && j == 1;
    double jump;
    if (KIND == 2) {
        // (the fp32 quotients K2d writes; Rayleigh's divisor is 1)
        const double ur = e[0] / q.dv, uz = e[q.e_plane] / q.dv, tz = e[2 * q.e_plane] / q.dv, tr = e[3 * q.e_plane] / q.dv;
        const double eu = sea_floor ? thick_energy_liquid(uz, tz, up, q.k, q.om2) : thick_energy_rayleigh(ur, uz, tz, tr, up, q.k, q.om2);
        jump = eu - thick_energy_rayleigh(ur, uz, tz, tr, dn, q.k, q.om2);
    } else {
        float ut = e[0] / q.dv, tq = e[q.e_plane] / q.dv;
        if (fabsf(ut) < 1.0e-20f) {                          // Love's low-amplitude exclusion, as K2d applies it
            const float vh = layer_at(q.mdl, q.fs, (size_t)q.hs * q.B + q.b, q.lnT, q.hs == q.n - 1).b;
            if (dn.b >= vh) { ut = 0.0f; tq = 0.0f; }
        }
        const double eu = sea_floor ? 0.0 : thick_energy_love(ut, tq, up, q.k, q.om2);
        jump = eu - thick_energy_love(ut, tq, dn, q.k, q.om2);
    }
    *kj = q.fac * jump;
    const double r0 = (double)R0, p = (double)pwr_of(KIND);
    const double z_j = z_up + (double)h_up;
    const double r_up = r0 - z_up, r_j = r0 - z_j;
    double sv, sr, chain = 0.0;
    if (h_up > 0.0f) {                                       // the layer above, regular role: its bottom radius moves
        thick_shares<KIND>(q, j - 1, &sv, &sr);
        const double x = log(r_up / r_j), inv = 1.0 / r_j - 1.0 / r_up, d = -expm1(-p * x);      // d = 1 - (rb / rt)^p
        const double dif_rb = -1.0 / (r_j * r_j * inv) + 1.0 / (x * r_j);
        const double qqq_rb = -p * (1.0 - d) / (r_j * d) + 1.0 / (x * r_j);
        chain = sv * dif_rb + sr * qqq_rb;
    }
    thick_shares<KIND>(q, j, &sv, &sr);                      // the layer below: its top radius moves
    if (j == q.n - 1) {
        chain = chain + (sv * (-1.0 / r_j) + sr * (p / r_j));
    } else if (h_dn > 0.0f) {
        const double r_dn = r0 - (z_j + (double)h_dn);
        const double x = log(r_j / r_dn), inv = 1.0 / r_dn - 1.0 / r_j, d = -expm1(-p * x);
        const double dif_rt = 1.0 / (r_j * r_j * inv) - 1.0 / (x * r_j);
        const double qqq_rt = p / (r_j * d) - 1.0 / (x * r_j);
        chain = chain + (sv * dif_rt + sr * qqq_rt);
    }
    return *kj * r0 / r_j - chain;
}

// One workgroup = 64 consecutive stacks at one period (a lane is one unit; a wavefront reads consecutive words of every plane
// of both scratches and of the staged fields) x 4 wavefronts that take every fourth interface of a 64-layer tile.  The
// thicknesses come from the caller's model rows through LDS (read along the layers); every lane forms the depth of each
// interface for itself, the fp64 sum in layer order from the tile's base depth (ascending pre-pass, wavefront 0).  Tiles run
// from the deepest to the top: the four wavefronts leave dcdz_j (fp64) of the interfaces i0 + 1 .. i0 + 64 in LDS, wavefront 0
// adds them from the deepest up into the running sum it carries across the tiles in a register - dcdh[i] is the sum after
// interface i + 1 - and the rows leave through the 64 x 64 tile (row stride 65) as in K2b; dcdz one word further (dcdz[0] is
// zero).  No atomics on floating-point values, no per-thread arrays; the order of every sum is fixed.
// Zeros: below the unit's effective half space and beyond nlay, unsolved periods, bad stacks, degenerate exits (no deepest
// layer or no factor), dcdh[nlay - 1], dcdz[0].  A unit with a value that is not finite: both rows NaN, counted.
template <int KIND>
__global__ __launch_bounds__(256) void surfdisp_thickness_kernel(ThickArgs A)
{
    static_assert(SURFDISP_NLAY_MAX <= 256, "zbase holds four 64-layer tiles");
    __shared__ double dzt[64][65];
    __shared__ float ht[65][65];
    __shared__ double zbase[4][64];
    __shared__ int badf[64];
    const int B = A.B, P = A.P, Lmax = A.Lmax;
    const int nbb = (B + 63) / 64;
    const int k = blockIdx.x / nbb, b0 = (blockIdx.x % nbb) * 64;
    const size_t PB = (size_t)P * B, fs = (size_t)Lmax * B;
    const int bl = threadIdx.x % 64, wv = threadIdx.x / 64;
    const int b = b0 + bl;
    const bool live = b < B;
    const size_t un = (size_t)k * B + (live ? b : b0);        // (read only where live)
    const int ntile = (Lmax + 63) / 64;
    ThickUnit q = thick_unit(A.mdl, fs, B, live ? b : b0, 0, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, -1, 0.0f, -1, nullptr, 0, 0, nullptr, 0, 0);
    if (live) {
        const int ehs = A.ehs[un];
        q = thick_unit(A.mdl, fs, B, b, A.nl[b], A.per[k], A.c[un], A.u[un], ehs >= 0 ? A.esum[un] : 0.0f,
                       ehs >= 0 ? A.ediv[un] : 1.0f, ehs, A.kscale[un], A.khs[un],
                       A.escr + un, PB, (size_t)Lmax * PB, A.kscr + un, PB, (size_t)Lmax * PB);
    }
    if (threadIdx.x < 64) badf[threadIdx.x] = 0;
    // thicknesses of the tile's layers (and the first of the next tile) -> ht[layer][stack]; 0 beyond nlay
    auto load_h = [&](int i0, int rows) {
        for (int t = threadIdx.x; t < rows * 64; t += 256) {
            const int il = t % rows, bq = t / rows;
            float h = 0.0f;
            if (b0 + bq < B && i0 + il < A.nl[b0 + bq]) h = A.model[((size_t)(b0 + bq) * 5 + 3) * Lmax + i0 + il];
            ht[il][bq] = h;
        }
    };
    double zrun = 0.0;
    for (int t = 0; t < ntile; ++t) {                        // base depth of every tile
        load_h(t * 64, 64);
        __syncthreads();
        if (wv == 0) {
            zbase[t][bl] = zrun;
            for (int il = 0; il < 64; ++il) zrun = zrun + (double)ht[il][bl];
        }
        __syncthreads();
    }
    double carry = 0.0;                                      // (wavefront 0) sum of dcdz over the interfaces below
    bool bad = false;
    for (int t = ntile - 1; t >= 0; --t) {
        const int i0 = t * 64;
        load_h(i0, 65);
        __syncthreads();
        double z = zbase[t][bl];                             // depth of the top of layer i0 + il
        for (int il = 0; il < 64; ++il) {
            const float h_up = ht[il][bl];
            if ((il & 3) == wv) {
                const int j = i0 + il + 1;
                double dz = 0.0, kj;
                if (j <= q.hs) {
                    dz = thick_interface<KIND>(q, j, z, h_up, ht[il + 1][bl], &kj);
                    if (!(fabs(dz) <= 1.0e300)) bad = true;
                }
                dzt[il][bl] = dz;
            }
            z = z + (double)h_up;
        }
        __syncthreads();
        if (wv == 0) {
            for (int il = 63; il >= 0; --il) {
                carry = carry + dzt[il][bl];
                ht[il][bl] = (float)carry;                   // dcdh[i0 + il]
            }
        }
        __syncthreads();
        for (int s = threadIdx.x; s < 64 * 64; s += 256) {
            const int bq = s / 64, il = s % 64;
            if (b0 + bq < B) {
                const size_t row = ((size_t)(b0 + bq) * P + k) * Lmax;
                if (i0 + il < Lmax) A.dcdh[row + i0 + il] = ht[il][bq];
                if (A.dcdz) {
                    if (i0 + il + 1 < Lmax) A.dcdz[row + i0 + il + 1] = (float)dzt[il][bq];
                    if (i0 + il == 0) A.dcdz[row] = 0.0f;
                }
            }
        }
        __syncthreads();
    }
    if (bad) badf[bl] = 1;                                   // (every writer stores the same value)
    __syncthreads();
    if (wv == 0 && live && badf[bl] && A.n_nonfinite) atomicAdd(A.n_nonfinite, 1);
    for (int s = threadIdx.x; s < 64 * Lmax; s += 256) {     // (rare) NaN rows
        const int bq = s / Lmax, i = s % Lmax;
        if (b0 + bq < B && badf[bq]) {
            const size_t o = ((size_t)(b0 + bq) * P + k) * Lmax + i;
            A.dcdh[o] = __builtin_nanf("");
            if (A.dcdz) A.dcdz[o] = __builtin_nanf("");
        }
    }
}

// ====================================================================== K4: group-velocity kernels
// surfdisp_forward_group_kernels_device, behind the forward + partials launches (whose outputs it leaves as they are).
// Differentiating U = d omega / dk at fixed omega (Rodi et al. 1975):
//      dU/dm = (U/c) (2 - U/c) dc/dm - (U/c)^2 d(dc/dm)/d ln T,
// with dc/dm the mean of the phase partials at T (1 - dfrac) and T (1 + dfrac) and d(dc/dm)/d ln T their central difference.
// K4a surfdisp_shift_kernel: one lane per (shift, period, stack) unit finds the fundamental-mode root at the shifted period
//   from the first-order prediction c' = c (1 +- dfrac (c/U - 1))  ((omega/c) dc/domega = 1 - c/U), WITHOUT a scan: a window
//   around c' is sampled at five points; exactly one sign change brackets the root, none widens the window (at most
//   SD_SHIFT_WIDEN times), more than one - or a non-finite value - fails the unit (a mode osculation, a layer velocity in
//   between, an overflow: a failure flag, not a guess).  A sign change that disappears with the layer dropping frozen at the
//   bracket's upper end (the refine passes' rule) was a jump of the dropping, not a root: failed too.  The bracket is then
//   bisected to fp32 resolution.  The secular function is the production recursion (ray_step / ray_close; the step of
//   delta_love) on layer values rebuilt in registers from the staged fields: a freshly built stack at the shifted period, as
//   SURFDISP_INDEPENDENT builds one.  Rayleigh: also the ellipticity at the root, as surfdisp_ellip_kernel forms it.
// K4b surfdisp_group_kernel<KIND, true> at the shifted periods and roots (chain factors at those periods).
// K4c surfdisp_group_combine_kernel: the rule above on the two layer-major scratches -> the caller's rows.
#ifndef SD_SHIFT_WIDEN
#define SD_SHIFT_WIDEN 6
#endif
struct ShiftStack { const float *mdl; size_t fs; int B, b, n; float T, lnT; };
__device__ __forceinline__ LayerV shift_layer(const ShiftStack &q, int i)
{
    return layer_at(q.mdl, q.fs, (size_t)i * q.B + q.b, q.lnT, i == q.n - 1);
}
// drop_layers on the rebuilt stack
__device__ __forceinline__ int shift_drop(const ShiftStack &q, float c)
{
    const float dmax = FACT * c * q.T;
    int cnt = 0;
    float sum = 0.0f;
    for (int ii = 0; ii < q.n; ++ii) {
        const LayerV v = shift_layer(q, ii);
        sum = sum + ((c < v.b) ? v.d : 0.0f);
        cnt += (sum > dmax) ? 0 : 1;
    }
    const int mm = (cnt < q.n) ? cnt + 1 : q.n;
    return mm < 2 ? 2 : mm;
}
// delta_rayleigh on the rebuilt stack (the ellipticity kernel's loop): start 1 dispersion, 2 / 3 the ellipticity passes
__device__ __forceinline__ float shift_delta_rayleigh(const ShiftStack &q, float c, int mm, int start, float *mag = nullptr)
{
    const RTrial t = ray_trial(c, q.T);
    RState s{};
    float phi = 0.0f, rho_prev = 0.0f, rho_i = 0.0f;
    RLyr y{};
    const int last = mm - 1;
    for (int i = 0; i <= last; ++i) {
        const LayerV v = shift_layer(q, i);
        rho_prev = rho_i;
        rho_i = v.rho;
        y.sv = v.b; y.d = v.d;
        y.ia2 = wk_ia2(v.a);
        y.ib2 = wk_ib2(v.b);
        y.rat = (i > 0) ? wk_rat(rho_prev, rho_i) : 0.0f;
        if (i == 0) {
            s = ray_start(t, start, (start == 1) ? 0.0f : wk_irho(rho_i));
            if (last >= 1) ray_step<true>(s, t, y, start, phi);
        } else if (i < last) {
            ray_step<false>(s, t, y, start, phi);
        }
    }
    return ray_close(s, t, y, rho_i, (last >= 1) ? rho_prev : 0.0f, start, mag, mag != nullptr);
}
// delta_love on the rebuilt stack (its step, without the certificate)
__device__ __forceinline__ float shift_delta_love(const ShiftStack &q, float c, int mm)
{
#pragma clang fp contract(off)
    const float wvno = 6.2831853f * rcp_nr(c * q.T);
    const float csq = c * c;
    const int mh = mm - 1;
    const LayerV vh = shift_layer(q, mh);
    const float h0 = vh.rho * vh.b * vh.b;
    const float rb0 = sqrt_hw(fabsf(fmaf(csq, wk_ilove(vh.rho, vh.b) * vh.rho, -1.0f)));
    float ut = 1.0f, tt = h0 * rb0;
    for (int m = mh - 1; m >= 0; --m) {
        const LayerV v = shift_layer(q, m);
        if (v.b == 0.0f) continue;                         // water, surfa.f:152
        const float ih = wk_ilove(v.rho, v.b);
        const float arg = fmaf(csq, ih * v.rho, -1.0f);
        const float h = v.rho * v.b * v.b;
        const LCoef Q = layer_coef(-arg, wvno * v.d);
        const float yv = -Q.sinr, z = -Q.rsin, cosq = Q.cs;
        const float eut = fmaf(cosq, ut, -(yv * tt * ih));
        const float ett = fmaf(h * z, ut, cosq * tt);
        ut = eut; tt = ett;
    }
    return -tt;
}

template <int KIND>
__global__ __launch_bounds__(256) void surfdisp_shift_kernel(ShiftArgs A)
{
    const int B = A.B, P = A.P;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // [2][P][B]: a wavefront = 64 stacks, one period
    if (idx >= (size_t)2 * P * B) return;
    const int b = (int)(idx % B), k = (int)((idx / B) % P), sg = (int)(idx / ((size_t)P * B));
    const float T = A.per[k];
    const float Ts = T * (sg ? 1.0f + A.dfrac : 1.0f - A.dfrac);
    if (b == 0) A.pers[sg * P + k] = Ts;
    const size_t o = (size_t)k * B + b;
    const float c0 = A.c[o];
    float root = c0, ell = 0.0f;
    unsigned char bad = 0;
    const int n = A.nl[b];
    if (n >= 2 && k < A.nsolved[b]) {
        bad = 1;
        const float u0 = A.u[o];
        const ShiftStack q{A.mdl, (size_t)A.Lmax * B, B, b, n, Ts, logf(1.0f / Ts)};
        auto delta = [&](float c, int mm) { return KIND == 2 ? shift_delta_rayleigh(q, c, mm, 1) : shift_delta_love(q, c, mm); };
        const float pred = c0 * (1.0f + (sg ? A.dfrac : -A.dfrac) * (c0 / u0 - 1.0f));
        float lo = 0.0f, hi = 0.0f, flo = 0.0f, fhi = 0.0f;
        bool found = false, broken = !(u0 > 0.0f) || !(pred > 0.0f) || !fin(pred);
        float hw = 0.25f * fabsf(pred - c0) + 1.0e-4f * c0;   // the prediction's error is second order in dfrac
        for (int it = 0; it <= SD_SHIFT_WIDEN && !found && !broken; ++it, hw *= 2.0f) {
            int changes = 0;
            float xp = 0.0f, fp = 0.0f;
            for (int j = 0; j < 5; ++j) {
                const float x = pred + (0.5f * (float)(j - 2)) * hw;
                if (!(x > 0.0f)) { broken = true; break; }
                const float f = delta(x, shift_drop(q, x));      // idrop = 0, as a scan trial
                if (!fin(f)) { broken = true; break; }
                if (j > 0 && ((f < 0.0f) != (fp < 0.0f))) { ++changes; lo = xp; flo = fp; hi = x; fhi = f; }
                xp = x; fp = f;
            }
            if (!broken && changes > 1) broken = true;
            found = !broken && changes == 1;
        }
        if (found) {
            const int mm = shift_drop(q, hi);                    // frozen, as the refine passes see it
            flo = delta(lo, mm);
            if (!fin(flo) || ((flo < 0.0f) == (fhi < 0.0f))) found = false;
            for (int it = 0; found && it < 48; ++it) {
                const float mid = 0.5f * (lo + hi);
                if (!(mid > lo && mid < hi)) break;
                const float f = delta(mid, mm);
                if (!fin(f)) { found = false; break; }
                if ((f < 0.0f) == (flo < 0.0f)) { lo = mid; flo = f; } else { hi = mid; fhi = f; }
            }
            if (found) {
                float r = lo - flo * ((hi - lo) / (fhi - flo));
                if (!(r >= lo && r <= hi)) r = 0.5f * (lo + hi);
                root = r;
                bad = 0;
                if (KIND == 2) {
                    float m2 = 0.0f, m3 = 0.0f;
                    float v2 = shift_delta_rayleigh(q, root, mm, 2, &m2), v3 = shift_delta_rayleigh(q, root, mm, 3, &m3);
                    const float b2max = A.ovf ? 0.5f * __expf(0.25f * A.ovf[2 * (size_t)B + b]) : 0.0f;
                    if ((A.ell_ambig < 0.0f) ||
                        ((A.ell_ambig > 0.0f) && (fabsf(v2) < A.ell_ambig * m2 || fabsf(v3) < A.ell_ambig * m3 ||
                                                  2.0f * b2max > A.ell_gmax * root * root))) {
                        auto get = [&](int m) { const LayerV v = shift_layer(q, m); return RefLyr{v.a, v.b, v.rho, v.d}; };
                        v2 = delta_rayleigh_ref_gen(get, mm, root, Ts, 2);
                        v3 = delta_rayleigh_ref_gen(get, mm, root, Ts, 3);
                    }
                    ell = 0.5f * v3 / v2;                        // surfa.f:363
                }
            }
        }
        if (bad) root = c0;                                      // (the partials pass runs on it; the combination writes NaN)
    }
    A.cs[idx] = root;
    if (A.ratio) A.ratio[idx] = ell;
    A.fail[idx] = bad;
}

// K4c: Rodi's rule (rodi_unit, surfdisp_k_rows.h) on the two shifted scratches, to the caller's rows (rows_through_tile).  A
// unit without phase partials (factor 0 at T: unsolved) gets a row of zeros, a solved unit whose shifted pass failed a row of
// NaN and is counted.  blockIdx.z: 0 dU/dVs, 1 dU/dVp, 2 dU/drho.
__global__ __launch_bounds__(256) void surfdisp_group_combine_kernel(GroupCombineArgs A)
{
    const int B = A.B, P = A.P, Lmax = A.Lmax;
    float *__restrict__ out = (blockIdx.z == 0) ? A.ub : ((blockIdx.z == 1) ? A.ua : A.ur);
    if (!out) return;                                        // (block-uniform)
    const size_t PB = (size_t)P * B;
    const float *__restrict__ sm = A.kscr_m + (size_t)blockIdx.z * Lmax * PB;
    const float *__restrict__ sp = A.kscr_p + (size_t)blockIdx.z * Lmax * PB;
    const bool zero_only = (blockIdx.z == 1) && (A.kind != 2);   // Love has no dU/dVp
    const RowTile t = row_tile(B);
    RodiUnit r{RODI_ZEROS, 0.0f, 0.0f};
    float scm = 0.0f, scp = 0.0f;
    int hsm = -1, hsp = -1;
    if (t.live && !zero_only) {
        r = rodi_unit(A.ksc0, A.ksc_m, A.ksc_p, A.fail, A.c, A.u, A.inv_dlnT, t.un, PB);
        if (r.state != RODI_ZEROS) {                         // (with the words rodi_unit reads, not behind its verdict)
            scm = A.ksc_m[t.un]; scp = A.ksc_p[t.un];
            hsm = A.khs_m[t.un]; hsp = A.khs_p[t.un];
        }
        if (r.state == RODI_NAN && A.n_failed && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < 64) atomicAdd(A.n_failed, 1);
    }
    rows_through_tile(t, B, P, Lmax, out, [&](int i) {
        float v = 0.0f;
        if (r.state == RODI_NAN) {
            v = __builtin_nanf("");
        } else if (r.state == RODI_COMBINE) {
            const size_t q = (size_t)i * PB + t.un;
            const float km = (i <= hsm) ? sm[q] * scm : 0.0f;
            const float kp = (i <= hsp) ? sp[q] * scp : 0.0f;
            v = r.f1 * (km + kp) - r.f2 * (kp - km);
        }
        return v;
    });
}

}  // namespace sd

// ======================================================================================= launch
namespace {

constexpr int SD_MAX_DEVICES = 64;

template <int KIND, int G, bool INDEP, bool FAST = false, bool EXACT = false>
hipError_t launch_phase_g(hipStream_t s, const sd::PhaseArgs &a)
{
    constexpr int S = SD_PHASE_BLOCK / G;
    const size_t lds = sd::phase_lds_bytes(a.Lmax, G, KIND);
    auto kern = sd::surfdisp_phase_kernel<KIND, G, INDEP, FAST, EXACT>;
    // raise the dynamic-LDS limit of this instantiation only when a launch needs more than any before it (per
    // device): the attribute call costs ~10 us, visible in launch-bound Metropolis loops
    static std::atomic<size_t> lds_set[SD_MAX_DEVICES];
    int dev = 0;
    (void)hipGetDevice(&dev);
    const int di = (dev >= 0 && dev < SD_MAX_DEVICES) ? dev : 0;
    if (lds > lds_set[di].load(std::memory_order_acquire) || dev != di) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        size_t cur = lds_set[di].load(std::memory_order_relaxed);
        while (lds > cur && !lds_set[di].compare_exchange_weak(cur, lds, std::memory_order_release)) {}
    }
    const long teams = INDEP ? (long)a.B * a.P : (long)a.B;
    const int grid = (int)((teams + S - 1) / S);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(SD_PHASE_BLOCK), lds, s, a);
    return hipGetLastError();
}

// the exact fallback: teams of 16 lanes, or as many as it takes for the working stacks to fit 64 KB of LDS
template <int KIND, bool INDEP>
hipError_t launch_phase_x(hipStream_t s, const sd::PhaseArgs &a)
{
    switch (sd::phase_exact_team(a.Lmax, KIND)) {
        case 16: return launch_phase_g<KIND, 16, INDEP, false, true>(s, a);
        case 32: return launch_phase_g<KIND, 32, INDEP, false, true>(s, a);
        default: return launch_phase_g<KIND, 64, INDEP, false, true>(s, a);
    }
}

template <int KIND, bool INDEP>
hipError_t launch_phase_k(hipStream_t s, const sd::PhaseArgs &a, int G)
{
    if (a.fast) {                                  // count-guided coarse scan: teams of 2..8 lanes only
        switch (G) {
            case 2:  return launch_phase_g<KIND, 2, INDEP, true>(s, a);
            case 4:  return launch_phase_g<KIND, 4, INDEP, true>(s, a);
            case 8:  return launch_phase_g<KIND, 8, INDEP, true>(s, a);
            default: break;
        }
    }
    switch (G) {
        case 1:  return launch_phase_g<KIND, 1, INDEP>(s, a);
        case 2:  return launch_phase_g<KIND, 2, INDEP>(s, a);
        case 4:  return launch_phase_g<KIND, 4, INDEP>(s, a);
        case 8:  return launch_phase_g<KIND, 8, INDEP>(s, a);
        case 16: return launch_phase_g<KIND, 16, INDEP>(s, a);
        case 32: return launch_phase_g<KIND, 32, INDEP>(s, a);
        case 64: return launch_phase_g<KIND, 64, INDEP>(s, a);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

namespace sd {

// one working stack per team + NEVILL's table x(12), y(12) behind the working stacks (the exact fallback: the same layout)
size_t phase_lds_bytes(int Lmax, int G, int kind) { const int S = SD_PHASE_BLOCK / G; return ((size_t)lds_ls(S, kind == 1 ? NFW_LOVE : NFW) * Lmax + (size_t)24 * S) * sizeof(float); }
int phase_exact_team(int Lmax, int kind)
{
    int G = 16;
    while (G < 64 && phase_lds_bytes(Lmax, G, kind) > 64u * 1024u) G *= 2;
    return G;
}

hipError_t launch_phase_exact(hipStream_t s, int kind, bool independent, const PhaseArgs &a)
{
    if (independent) return kind == 2 ? launch_phase_x<2, true>(s, a) : launch_phase_x<1, true>(s, a);
    return kind == 2 ? launch_phase_x<2, false>(s, a) : launch_phase_x<1, false>(s, a);
}

template <int KIND>
static void launch_prep_k(hipStream_t s, int TL, const PrepArgs &a)
{
    const long threads = (long)a.B * TL;
    const int grid = (int)((threads + 255) / 256);
    switch (TL) {
        case 1:  hipLaunchKernelGGL((surfdisp_prep_kernel<KIND, 1>), dim3(grid), dim3(256), 0, s, a); break;
        case 2:  hipLaunchKernelGGL((surfdisp_prep_kernel<KIND, 2>), dim3(grid), dim3(256), 0, s, a); break;
        case 4:  hipLaunchKernelGGL((surfdisp_prep_kernel<KIND, 4>), dim3(grid), dim3(256), 0, s, a); break;
        case 8:  hipLaunchKernelGGL((surfdisp_prep_kernel<KIND, 8>), dim3(grid), dim3(256), 0, s, a); break;
        case 16: hipLaunchKernelGGL((surfdisp_prep_kernel<KIND, 16>), dim3(grid), dim3(256), 0, s, a); break;
        case 32: hipLaunchKernelGGL((surfdisp_prep_kernel<KIND, 32>), dim3(grid), dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((surfdisp_prep_kernel<KIND, 64>), dim3(grid), dim3(256), 0, s, a); break;
    }
}

hipError_t launch_prep(hipStream_t s, int kind, const PrepArgs &a)
{
    // lanes per stack: enough wavefronts to give every SIMD about four (262 144 lanes), never more lanes than layers
    int TL = 1;
    while (TL < 64 && (long)a.B * TL < 262144L && TL < a.Lmax) TL *= 2;
    if (kind == 2) launch_prep_k<2>(s, TL, a); else launch_prep_k<1>(s, TL, a);
    return hipGetLastError();
}

hipError_t launch_phase(hipStream_t s, int kind, int G, bool independent, const PhaseArgs &a)
{
    if (independent) return kind == 2 ? launch_phase_k<2, true>(s, a, G) : launch_phase_k<1, true>(s, a, G);
    return kind == 2 ? launch_phase_k<2, false>(s, a, G) : launch_phase_k<1, false>(s, a, G);
}

hipError_t launch_kern_transpose(hipStream_t s, const KernTransposeArgs &a)
{
    hipLaunchKernelGGL(surfdisp_kern_transpose_kernel, rows_grid(a.B, a.P, a.Lmax, 3u), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_eigen_transpose(hipStream_t s, const EigenTransposeArgs &a)
{
    hipLaunchKernelGGL(surfdisp_eigen_transpose_kernel, rows_grid(a.B, a.P, a.Lmax, 4u), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_atten(hipStream_t s, const AttenArgs &a)
{
    const dim3 grid((unsigned)(a.P * ((a.B + 63) / 64)));
    if (a.kind == 2) hipLaunchKernelGGL((surfdisp_atten_kernel<2>), grid, dim3(256), 0, s, a);
    else             hipLaunchKernelGGL((surfdisp_atten_kernel<1>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_thickness(hipStream_t s, const ThickArgs &a)
{
    const dim3 grid((unsigned)(a.P * ((a.B + 63) / 64)));
    if (a.kind == 2) hipLaunchKernelGGL((surfdisp_thickness_kernel<2>), grid, dim3(256), 0, s, a);
    else             hipLaunchKernelGGL((surfdisp_thickness_kernel<1>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_shift(hipStream_t s, const ShiftArgs &a)
{
    const size_t total = (size_t)2 * a.B * a.P;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (a.kind == 2) hipLaunchKernelGGL((surfdisp_shift_kernel<2>), grid, dim3(256), 0, s, a);
    else             hipLaunchKernelGGL((surfdisp_shift_kernel<1>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_combine(hipStream_t s, const GroupCombineArgs &a)
{
    hipLaunchKernelGGL(surfdisp_group_combine_kernel, rows_grid(a.B, a.P, a.Lmax, 3u), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ellip(hipStream_t s, const EllipArgs &a)
{
    const size_t total = (size_t)a.B * a.P;
    hipLaunchKernelGGL(surfdisp_ellip_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_finish(hipStream_t s, const FinishArgs &a)
{
    const int grid = (a.B + 63) / 64;
    const size_t lds = (size_t)64 * (a.P + 1) * sizeof(float);
    hipLaunchKernelGGL(surfdisp_finish_kernel, dim3(grid), dim3(256), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_group(hipStream_t s, int kind, const GroupArgs &a_in)
{
    GroupArgs a = a_in;
    const size_t total = (size_t)a.B * a.P;
    int grid = (int)((total + 255) / 256);
    const bool kern = a.kb != nullptr;
    // Workgroup order (see the kernel).  group_order < 0 (default): the XCD-aware order, four stack blocks per XCD at a time, for the
    // launches that also write the partials when every XCD gets the same number (<= 8) of stack blocks; plain period-major order
    // otherwise.  Measured (16 384 x L64 / 25 600 x L96, P20, Rayleigh; profiles/r04b/group_order.txt): with the partials
    // 535 us + 808 MB fetched in plain order, 533 us + 216 MB with four blocks at a time, 565 us + 75 MB with one; without them
    // 471 / 502 / 499 us (the plain launch is not worth it); 25 600 stacks (12.5 blocks per XCD: uneven shares) 1.25 ms plain,
    // 1.39 .. 1.55 ms in every grouped order.
    const int nblk = (a.B + 255) / 256;
    int g = a.group_order;
    if (g < 0) g = (kern && a.B % 2048 == 0 && nblk / 8 <= 8) ? (nblk / 8 < 4 ? nblk / 8 : 4) : 0;
    a.krev = g >= 100 ? 1 : 0;
    g %= 100;
    a.xcd_order = (nblk >= 8 && a.B % 256 == 0 && g > 0) ? g : 0;
    if (a.xcd_order) grid = (((nblk + 7) / 8 + a.xcd_order - 1) / a.xcd_order) * a.xcd_order * 8 * a.P;
    // (the eigenfunction entry: the plain kernel's EIG instantiation; it writes no partials)
    if (a.escr && !kern) {
        if (kind == 2) hipLaunchKernelGGL((surfdisp_group_kernel<2, false, true>), dim3(grid), dim3(256), 0, s, a);
        else           hipLaunchKernelGGL((surfdisp_group_kernel<1, false, true>), dim3(grid), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (a.escr) return hipErrorInvalidValue;
    // The default Rayleigh launch keeps the fit's layer values in LDS for the later sweeps (LStash) while the three
    // workgroups per CU that its registers allow still fit in the CU's 160 KB: Lmax x SD_STASH_W KB each, Lmax <= 10.
    // Deeper batches, and a.stash < 0 (SURFDISP_GROUP_STASH=0, or a SURFDISP_PIPELINED call: beside other batches the
    // stash's LDS keeps their root-search workgroups off the CU - 65 536 x L10 x P20 with three batches in flight
    // 40.9 -> 36.5 M solves/s with it, profiles/r10a), derive them again in every sweep - the same bits.
    size_t lds = 0;
    a.stash = 0;
#ifndef SD_NO_GROUP_STASH
    if (kind == 2 && !kern && a_in.stash >= 0 && (size_t)a.Lmax * SD_STASH_W * 1024 * SD_GROUP_WAVES <= 160u * 1024u) {
        a.stash = 1;
        lds = (size_t)a.Lmax * SD_STASH_W * 256 * sizeof(float);
    }
#endif
    if (kind == 2 && kern)  hipLaunchKernelGGL((surfdisp_group_kernel<2, true>), dim3(grid), dim3(256), 0, s, a);
    else if (kind == 2 && a.stash) hipLaunchKernelGGL(surfdisp_group_kernel_stash, dim3(grid), dim3(256), lds, s, a);
    else if (kind == 2)     hipLaunchKernelGGL((surfdisp_group_kernel<2, false>), dim3(grid), dim3(256), 0, s, a);
    else if (kern)          hipLaunchKernelGGL((surfdisp_group_kernel<1, true>), dim3(grid), dim3(256), 0, s, a);
    else                    hipLaunchKernelGGL((surfdisp_group_kernel<1, false>), dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}


// ====================================================================== K5: ellipticity kernels
// surfdisp_forward_ellip_kernels_device, behind the forward + partials launches (whose outputs it leaves as they are).
// The ellipticity is chi = D(e3) / (2 D(e2)) with D(e) = h^T A_{last-1} ... A_0 e the reference's layer recursion (DLTAR4,
// surfa.f:193-363) on the working stack the root search left (replayed from the hist words as surfdisp_ellip_kernel does; a
// liquid top layer is skipped by the two ellipticity passes), and the root obeys F = D(e1) = 0.  At the root
//     dchi/dm_i = (dD3_i - 2 chi dD2_i) / (2 D2) + gamma dF_i,   gamma = -(dchi/dc) / (dF/dc),
// where dD(e)_i = u_i (dA_i/dm_i) v_{i-1}(e) contracts the adjoint row u_i = h^T A_{last-1} ... A_{i+1} with the forward state
// v_{i-1}(e) = A_{i-1} ... A_0 e (the half space: dh/dm v_{last-1}), and d/dc sums such terms over every layer - the liquid
// top layer's included for F.  fp64 throughout; the layer matrix is written with C(z) = cos sqrt(z), S(z) = sin sqrt(z) /
// sqrt(z) of z = d^2 (omega^2 / a^2 - k^2) (entire functions: cosh / sinh for z < 0, a series near 0), so it is smooth
// across c = a or b, and its derivatives come from one dual-number evaluation per direction (a, b, rho, c).
// One lane per (stack, period) unit, three sweeps: K5a the layer history (which period last refreshed each layer), K5b the
// adjoint rows upward into a layer-major scratch [5][Lmax][P*B] (fp64), K5c downward: forward states of e1, e2, e3, the
// contractions, the chain factors of calcul.f:122-126 / flat1.f:44-62 at the refreshing period - the two per-layer shares
// (dchi/dm at fixed c, dF/dm) go to layer-major fp32 scratches, gamma and the deepest layer to per-unit words.
// K5d surfdisp_ellip_transpose_kernel: share + gamma x F-share -> the caller's rows (zeros below the half space; NaN rows).
struct Dd { double v, d; };
__device__ __forceinline__ Dd operator+(Dd x, Dd y) { return Dd{x.v + y.v, x.d + y.d}; }
__device__ __forceinline__ Dd operator-(Dd x, Dd y) { return Dd{x.v - y.v, x.d - y.d}; }
__device__ __forceinline__ Dd operator-(Dd x) { return Dd{-x.v, -x.d}; }
__device__ __forceinline__ Dd operator*(Dd x, Dd y) { return Dd{x.v * y.v, x.v * y.d + x.d * y.v}; }
__device__ __forceinline__ Dd operator/(Dd x, Dd y) { const double q = x.v / y.v; return Dd{q, (x.d - q * y.d) / y.v}; }
__device__ __forceinline__ Dd operator*(double s, Dd x) { return Dd{s * x.v, s * x.d}; }
__device__ __forceinline__ Dd operator+(double s, Dd x) { return Dd{s + x.v, x.d}; }
__device__ __forceinline__ Dd operator-(double s, Dd x) { return Dd{s - x.v, -x.d}; }
__device__ __forceinline__ Dd operator-(Dd x, double s) { return Dd{x.v - s, x.d}; }
__device__ __forceinline__ Dd operator/(double s, Dd x) { const double q = s / x.v; return Dd{q, -q * x.d / x.v}; }
__device__ __forceinline__ double dval(double x) { return x; }
__device__ __forceinline__ double dval(Dd x) { return x.v; }
__device__ __forceinline__ double dder(double) { return 0.0; }
__device__ __forceinline__ double dder(Dd x) { return x.d; }
__device__ __forceinline__ double dsqrt(double x) { return sqrt(x); }
__device__ __forceinline__ Dd dsqrt(Dd x) { const double r = sqrt(x.v); return Dd{r, 0.5 * x.d / r}; }
// C(z), S(z) and their z-derivatives (C' = -S/2, S' = (C - S) / (2 z); series for |z| < 1, where that quotient cancels)
struct CSv { double C, S, dC, dS; };
// sin and cos of q >= 0 (q = sqrt(z) stays far below 2^20 wherever the recursion is finite): Cody-Waite reduction by pi/2 in
// three parts and Taylor polynomials on [-pi/4, pi/4] (the library's fp64 sin / cos keep a private array for huge arguments)
__device__ __forceinline__ void ell_sincos(double q, double *sn, double *cn)
{
    const double n = rint(q * 0.63661977236758134308);
    const double r = ((q - n * 1.57079632673412561417e+00) - n * 6.07710050630396597660e-11) - n * 2.02226624879595063154e-21;
    const double r2 = r * r;
    double ps = 1.0, pc = 1.0;                              // Horner, inside out: 1 - r^2 / ((2m) (2m+1)) (...), 1 - r^2 / ((2m-1) 2m) (...)
#pragma unroll
    for (int m = 10; m >= 1; --m) {
        ps = 1.0 - r2 * ps / ((2.0 * m) * (2.0 * m + 1.0));
        pc = 1.0 - r2 * pc / ((2.0 * m - 1.0) * (2.0 * m));
    }
    const double sr = r * ps, cr = pc;
    const int j = (int)((long long)n & 3);
    *sn = (j == 0) ? sr : ((j == 1) ? cr : ((j == 2) ? -sr : -cr));
    *cn = (j == 0) ? cr : ((j == 1) ? -sr : ((j == 2) ? -cr : sr));
}
__device__ __forceinline__ CSv cs_of(double z)
{
    CSv r;
    if (fabs(z) < 1.0) {
        double t = 1.0, C = 0.0, S = 0.0, dS = 0.0;             // t = (-z)^n
        double fc = 1.0, fs = 1.0;                              // 1 / (2n)!, 1 / (2n+1)!
#pragma unroll
        for (int m = 0; m < 11; ++m) {
            C += t * fc; S += t * fs;
            if (m < 10) dS -= (double)(m + 1) * t * fs / ((2.0 * m + 2.0) * (2.0 * m + 3.0));   // (n+1) (-z)^n (-1) / (2n+3)!
            t *= -z;
            fc /= (2.0 * m + 1.0) * (2.0 * m + 2.0);
            fs /= (2.0 * m + 2.0) * (2.0 * m + 3.0);
        }
        r.C = C; r.S = S; r.dS = dS;
    } else if (z > 0.0) {
        const double q = sqrt(z);
        double sn, cn; ell_sincos(q, &sn, &cn);
        r.C = cn; r.S = sn / q; r.dS = (r.C - r.S) / (2.0 * z);
    } else {
        const double q = sqrt(-z), e = exp(q), ie = 1.0 / e;
        r.C = 0.5 * (e + ie); r.S = 0.5 * (e - ie) / q; r.dS = (r.C - r.S) / (2.0 * z);
    }
    r.dC = -0.5 * r.S;
    return r;
}
__device__ __forceinline__ double cs_lift(double v, double, double) { return v; }
__device__ __forceinline__ Dd cs_lift(double v, double dv, Dd z) { return Dd{v, dv * z.d}; }
template <class T> struct EMat { T a11, a12, a13, a14, a15, a21, a22, a23, a24, a31, a32, a33, a41, a42, a51; };
struct EV5 { double x[5]; };
// z of the P and S phases of a layer (values only: what cs_of is evaluated at)
__device__ __forceinline__ void ell_z(double a, double b, double d, double c, double k, double *za, double *zb)
{
    const double kd2 = (k * d) * (k * d), csq = c * c;
    *za = -(1.0 - csq / (a * a)) * kd2;
    *zb = (b > 0.0) ? -(1.0 - csq / (b * b)) * kd2 : 0.0;
}
// the layer matrix of DLTAR4 (surfa.f:253-357; liquid: 216-251) in the C / S form
template <class T>
__device__ __forceinline__ EMat<T> ell_mat(T a, T b, T rho, T d, T c, T k, const CSv &ca, const CSv &cb, bool liquid)
{
    const T csq = c * c, kd = k * d;
    const T arga = 1.0 - csq / (a * a);
    const T za = -(arga * kd * kd);
    const T Sa = cs_lift(ca.S, ca.dS, za);
    const T cosp = cs_lift(ca.C, ca.dC, za), sinpr = kd * Sa, rsinp = -(arga * kd * Sa);
    const T rhoc = rho * csq;
    // (one straight path, the liquid case selected per entry: two return paths put the matrix in private memory)
    const T argb = 1.0 - csq / (b * b);
    const T zb = -(argb * kd * kd);
    const T Sb = cs_lift(cb.S, cb.dS, zb);
    const T cosq = cs_lift(cb.C, cb.dC, zb), sinqr = kd * Sb, rsinq = -(argb * kd * Sb);
    const T g = 2.0 * (b * b) / csq, g1 = g - 1.0;
    const T rr = rsinp * rsinq, ss = sinpr * sinqr, cc = cosp * cosq;
    const T rs1 = rsinp * cosq, rs2 = sinqr * cosp, rs3 = sinpr * cosq, rs4 = rsinq * cosp;
    const T gm = 2.0 * g - 1.0, gs = g * g, g1s = g1 * g1, ccm = 1.0 - cc, gg1 = g * g1;
    const T rhocs = rhoc * rhoc;
    const T suu = gs * rr + g1s * ss;
    const T z = csq - csq;
    EMat<T> m;
    m.a11 = liquid ? cosp : (2.0 * gs - gm) * cc - suu - 2.0 * gg1;
    m.a12 = liquid ? z : -(rs1 + rs2) / rhoc;
    m.a13 = liquid ? z : -2.0 * (gm * ccm + g1 * ss + g * rr) / rhoc;
    m.a14 = liquid ? z : (rs3 + rs4) / rhoc;
    m.a15 = liquid ? z : (2.0 * ccm + rr + ss) / rhocs;
    m.a21 = liquid ? rhoc * sinpr : rhoc * (g1s * rs3 + gs * rs4);
    m.a22 = liquid ? z : cc;
    m.a23 = liquid ? z : 2.0 * (g * rs4 + g1 * rs3);
    m.a24 = liquid ? z : sinpr * rsinq;
    m.a31 = liquid ? z : rhoc * (gg1 * gm * ccm + g1s * g1 * ss + gs * g * rr);
    m.a32 = liquid ? z : g1 * rs2 + g * rs1;
    m.a33 = liquid ? z : 1.0 + 2.0 * (2.0 * gg1 * ccm + suu);
    m.a41 = liquid ? z : -(rhoc * (g1s * rs2 + gs * rs1));
    m.a42 = liquid ? z : rsinp * sinqr;
    m.a51 = liquid ? z : rhocs * (2.0 * gs * g1s * ccm + gs * gs * rr + g1s * g1s * ss);
    return m;
}
// the half-space row h (label 52 of DLTAR4, surfa.f:346-363), the factor 2 of h13 folded in
template <class T>
__device__ __forceinline__ void ell_hrow(T a, T b, T rho, T c, T h[5])
{
    const T csq = c * c;
    const T arga = 1.0 - csq / (a * a), argb = 1.0 - csq / (b * b);
    const T ra = (dval(arga) > 0.0) ? -dsqrt(arga) : dsqrt(0.0 - arga);
    const T rb = (dval(argb) > 0.0) ? -dsqrt(argb) : dsqrt(0.0 - argb);
    const T g = 2.0 * (b * b) / csq, g1 = g - 1.0;
    const T sss = b * b, ppp = a * a, rhp = rho * a;
    const T gra = g * ra, rba = rb - 1.0 / ra;
    const T h12r = rhp * a;
    h[0] = -2.0 * rb * sss / ppp + csq * (g1 * g1) / ppp / gra;
    h[1] = -1.0 / g / h12r;
    h[2] = 2.0 * (-rb / h12r + g1 / h12r / gra);
    h[3] = rb / h12r / gra;
    h[4] = rba / rhp / rhp / csq / g;
}
template <bool DER, class T>
__device__ __forceinline__ EV5 ell_act(const EMat<T> &A, const EV5 &b)
{
    auto e = [](const T &x) { return DER ? dder(x) : dval(x); };
    const double a11 = e(A.a11), a12 = e(A.a12), a13 = e(A.a13), a14 = e(A.a14), a15 = e(A.a15), a21 = e(A.a21), a22 = e(A.a22),
                 a23 = e(A.a23), a24 = e(A.a24), a31 = e(A.a31), a32 = e(A.a32), a33 = e(A.a33), a41 = e(A.a41), a42 = e(A.a42),
                 a51 = e(A.a51);
    const double b1 = b.x[0], b2 = b.x[1], b3 = b.x[2], b4 = b.x[3], b5 = b.x[4];
    EV5 r;
    r.x[0] = a11 * b1 + a12 * b2 + a13 * b3 + a14 * b4 + a15 * b5;
    r.x[1] = a21 * b1 + a22 * b2 + a23 * b3 + a24 * b4 - a14 * b5;
    r.x[2] = a31 * b1 + a32 * b2 + a33 * b3 - 0.5 * a23 * b4 + 0.5 * a13 * b5;
    r.x[3] = a41 * b1 + a42 * b2 - 2.0 * a32 * b3 + a22 * b4 - a12 * b5;
    r.x[4] = a51 * b1 - a41 * b2 + 2.0 * a31 * b3 - a21 * b4 + a11 * b5;
    return r;
}
// the row u A (the adjoint step)
__device__ __forceinline__ EV5 ell_act_row(const EMat<double> &A, const EV5 &u)
{
    const double u1 = u.x[0], u2 = u.x[1], u3 = u.x[2], u4 = u.x[3], u5 = u.x[4];
    EV5 r;
    r.x[0] = A.a11 * u1 + A.a21 * u2 + A.a31 * u3 + A.a41 * u4 + A.a51 * u5;
    r.x[1] = A.a12 * u1 + A.a22 * u2 + A.a32 * u3 + A.a42 * u4 - A.a41 * u5;
    r.x[2] = A.a13 * u1 + A.a23 * u2 + A.a33 * u3 - 2.0 * A.a32 * u4 + 2.0 * A.a31 * u5;
    r.x[3] = A.a14 * u1 + A.a24 * u2 - 0.5 * A.a23 * u3 + A.a22 * u4 - A.a21 * u5;
    r.x[4] = A.a15 * u1 - A.a14 * u2 + 0.5 * A.a13 * u3 - A.a12 * u4 + A.a11 * u5;
    return r;
}
__device__ __forceinline__ double ell_dot(const EV5 &u, const EV5 &v)
{
    return u.x[0] * v.x[0] + u.x[1] * v.x[1] + u.x[2] * v.x[2] + u.x[3] * v.x[3] + u.x[4] * v.x[4];
}
__device__ __forceinline__ bool finite64(double x) { return fabs(x) <= 1.7976931348623157e308; }

// one working-stack layer of unit (b, k): its values, as the rebuild of period kk formed them, and their chain factors
struct ELayer { double a, b, rho, d; Chain ch; bool liquid; };
__device__ __forceinline__ ELayer ell_layer(const EllipKernArgs &A, int b, int i, int kpk)
{
    const size_t fs = (size_t)A.Lmax * A.B;
    const LayerRaw raw = layer_load(A.mdl, fs, (size_t)i * A.B + b);
    const float lnT = logf(1.0f / A.per[kpk & 0xffff]);
    const bool hs = (kpk & 0x10000) != 0;
    const LayerV v = layer_derive(raw, lnT, hs);
    ELayer e;
    e.a = v.a; e.b = v.b; e.rho = v.rho; e.d = v.d;
    e.ch = chain_of(raw, lnT, hs, false);
    e.liquid = !(fabsf(v.b) > 1.e-8f);                      // DLTAR4's test, surfa.f:216
    return e;
}

__global__ __launch_bounds__(256) void surfdisp_ellip_kern_kernel(EllipKernArgs A)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int B = A.B, P = A.P;
    if (idx >= (size_t)B * P) return;
    const int b = (int)(idx % B), k = (int)(idx / B);       // a wavefront = 64 stacks, one period: coalesced scratch
    const size_t PB = (size_t)P * B;
    const int n = A.nl[b];
    int top = -1;                                           // deepest layer with partials; -2: NaN row
    float gam = 0.0f;
    const int hk = (n >= 2 && k < A.nsolved[b] && A.c[idx] > 0.0f) ? A.hist[idx] : 0x7fffffff;
    if (hk == 0x7fffffff) {
        // unsolved period or bad stack: zeros
    } else if (((hk >> 16) & 0x3fff) < 2 || ((hk >> 16) & 0x3fff) > n) {
        top = -2;                                           // (no recursion to differentiate)
    } else {
        const int last = ((hk >> 16) & 0x3fff) - 1;         // the half space of the recursion (frozen mmax - 1)
        // K5a: which period's rebuild the working stack's layer i comes from (surfdisp_ellip_kernel's replay)
        {
            int kk = k, nflat = hk & 0xffff;
            for (int i = 0; i <= last; ++i) {
                while (nflat <= i && kk > 0) {
                    --kk;
                    nflat = A.hist[(size_t)kk * B + b] & 0xffff;      // (periods the exact kernel solved: sign bit set)
                }
                A.kpk[(size_t)i * PB + idx] = kk | ((i == nflat - 1) ? 0x10000 : 0);
            }
        }
        const double c = A.c[idx], T = A.per[k];
        const double kw = 6.283185307179586 / (c * T);       // wavenumber
        // K5b: adjoint rows, upward.  u_{last-1} = h; u_{i-1} = u_i A_i
        EV5 u;
        ELayer hl = ell_layer(A, b, last, A.kpk[(size_t)last * PB + idx]);
        {
            double h[5];
            ell_hrow<double>(hl.a, hl.b, hl.rho, c, h);
            for (int q = 0; q < 5; ++q) u.x[q] = h[q];
        }
        for (int i = last - 1; i >= 0; --i) {
            for (int q = 0; q < 5; ++q) A.wscr[((size_t)q * A.Lmax + i) * PB + idx] = u.x[q];
            const ELayer L = ell_layer(A, b, i, A.kpk[(size_t)i * PB + idx]);
            double za, zb; ell_z(L.a, L.b, L.d, c, kw, &za, &zb);
            const CSv ca = cs_of(za), cb = cs_of(zb);
            const EMat<double> M = ell_mat<double>(L.a, L.b, L.rho, L.d, c, kw, ca, cb, L.liquid && i == 0);
            u = ell_act_row(M, u);
        }
        // u is now u_{-1} = h A_{last-1} ... A_0: D(e) = u_{-1} e, or - liquid top layer, skipped by the ellipticity passes -
        // u_0 e
        const bool wtop = (last >= 1) && ell_layer(A, b, 0, A.kpk[idx]).liquid;
        double D2, D3;
        if (wtop) {
            D2 = A.wscr[((size_t)1 * A.Lmax + 0) * PB + idx];
            D3 = A.wscr[((size_t)2 * A.Lmax + 0) * PB + idx];
        } else {
            D2 = u.x[1]; D3 = u.x[2];
        }
        const double chi = 0.5 * D3 / D2;
        const double i2D2 = 0.5 / D2;
        // K5c: forward states of e1, e2, e3, downward, and the contractions
        EV5 v1{{1.0, 0.0, 0.0, 0.0, 0.0}}, v2{{0.0, 1.0, 0.0, 0.0, 0.0}}, v3{{0.0, 0.0, 1.0, 0.0, 0.0}};
        double Fc = 0.0, Xc = 0.0;                          // dF/dc, d(D3 - 2 chi D2)/dc at fixed chi
        bool ok = finite64(chi) && finite64(i2D2);
        const size_t arr = (size_t)A.Lmax * PB;
        for (int i = 0; i <= last; ++i) {
            const bool is_hs = (i == last);
            const ELayer L = is_hs ? hl : ell_layer(A, b, i, A.kpk[(size_t)i * PB + idx]);
            const bool liq = L.liquid && i == 0 && !is_hs;
            double sF[4] = {0.0, 0.0, 0.0, 0.0}, sX[4] = {0.0, 0.0, 0.0, 0.0};   // directions a, b, rho, c
            if (is_hs) {
#pragma unroll
                for (int dir = 0; dir < 4; ++dir) {
                    const Dd a{L.a, dir == 0 ? 1.0 : 0.0}, bb{L.b, dir == 1 ? 1.0 : 0.0}, r{L.rho, dir == 2 ? 1.0 : 0.0},
                             cc{c, dir == 3 ? 1.0 : 0.0};
                    Dd h[5];
                    ell_hrow<Dd>(a, bb, r, cc, h);
                    EV5 dh;
                    for (int q = 0; q < 5; ++q) dh.x[q] = h[q].d;
                    sF[dir] = ell_dot(dh, v1);
                    sX[dir] = ell_dot(dh, v3) - 2.0 * chi * ell_dot(dh, v2);
                }
            } else {
                EV5 ui;
                for (int q = 0; q < 5; ++q) ui.x[q] = A.wscr[((size_t)q * A.Lmax + i) * PB + idx];
                double za, zb; ell_z(L.a, L.b, L.d, c, kw, &za, &zb);
                const CSv ca = cs_of(za), cb = cs_of(zb);
                EMat<double> M{};
#pragma unroll
                for (int dir = 0; dir < 4; ++dir) {
                    if (liq && dir < 3) continue;
                    const Dd a{L.a, dir == 0 ? 1.0 : 0.0}, bb{L.b, dir == 1 ? 1.0 : 0.0}, r{L.rho, dir == 2 ? 1.0 : 0.0},
                             cc{c, dir == 3 ? 1.0 : 0.0}, kk{kw, dir == 3 ? -kw / c : 0.0}, d{L.d, 0.0};
                    const EMat<Dd> Md = ell_mat<Dd>(a, bb, r, d, cc, kk, ca, cb, liq);
                    sF[dir] = ell_dot(ui, ell_act<true>(Md, v1));
                    if (!liq) sX[dir] = ell_dot(ui, ell_act<true>(Md, v3)) - 2.0 * chi * ell_dot(ui, ell_act<true>(Md, v2));
                    if (dir == 3) {
#define SD_EV(f) M.f = Md.f.v
                        SD_EV(a11); SD_EV(a12); SD_EV(a13); SD_EV(a14); SD_EV(a15); SD_EV(a21); SD_EV(a22); SD_EV(a23);
                        SD_EV(a24); SD_EV(a31); SD_EV(a32); SD_EV(a33); SD_EV(a41); SD_EV(a42); SD_EV(a51);
#undef SD_EV
                    }
                }
                v1 = ell_act<false>(M, v1);
                if (!liq) { v2 = ell_act<false>(M, v2); v3 = ell_act<false>(M, v3); }
            }
            Fc += sF[3];
            Xc += sX[3];
            // flattened (a, b, rho) -> the caller's (Vs, Vp, rho) of input layer i; a liquid layer gets none
            const Chain ch = L.ch;
            const double xb = liq ? 0.0 : i2D2 * (sX[1] * ch.dbdb + sX[0] * ch.dadb), xa = liq ? 0.0 : i2D2 * sX[0] * ch.dada,
                         xr = liq ? 0.0 : i2D2 * sX[2] * ch.rfac;
            const double fb = liq ? 0.0 : sF[1] * ch.dbdb + sF[0] * ch.dadb, fa = liq ? 0.0 : sF[0] * ch.dada,
                         fr = liq ? 0.0 : sF[2] * ch.rfac;
            ok = ok && finite64(xb) && finite64(xa) && finite64(xr) && finite64(fb) && finite64(fa) && finite64(fr);
            const size_t o = (size_t)i * PB + idx;
            A.xscr[o] = (float)xb; A.xscr[arr + o] = (float)xa; A.xscr[2 * arr + o] = (float)xr;
            A.fscr[o] = (float)fb; A.fscr[arr + o] = (float)fa; A.fscr[2 * arr + o] = (float)fr;
        }
        // F-shares are stored unscaled; the unit's gamma = -(dchi/dc) / (dF/dc) carries 1 / (dF/dc)
        const double g = -(i2D2 * Xc) / Fc;
        ok = ok && finite64(g) && Fc != 0.0 && fabs(g) <= 3.0e38;
        top = ok ? last : -2;
        gam = ok ? (float)g : 0.0f;
    }
    A.gam[idx] = gam;
    A.khs[idx] = top;
    if (top == -2 && A.n_nonfinite) atomicAdd(A.n_nonfinite, 1);
}

// K5d: share + gamma x F-share -> the caller's [B][P][Lmax] rows (rows_through_tile, surfdisp_k_rows.h); zeros below the
// unit's half space and for units without partials, NaN for every entry of a non-finite unit (khs == -2).  blockIdx.z: 0
// dchi/dVs, 1 dchi/dVp, 2 dchi/drho.
__global__ __launch_bounds__(256) void surfdisp_ellip_transpose_kernel(EllipTransposeArgs A)
{
    const int B = A.B, P = A.P, Lmax = A.Lmax;
    float *__restrict__ out = (blockIdx.z == 0) ? A.eb : ((blockIdx.z == 1) ? A.ea : A.er);
    if (!out) return;                                        // (block-uniform)
    const size_t PB = (size_t)P * B;
    const float *__restrict__ xs = A.xscr + (size_t)blockIdx.z * Lmax * PB;
    const float *__restrict__ fsr = A.fscr + (size_t)blockIdx.z * Lmax * PB;
    const RowTile t = row_tile(B);
    float g = 0.0f; int hs = -1;
    if (t.live) { g = A.gam[t.un]; hs = A.khs[t.un]; }
    rows_through_tile(t, B, P, Lmax, out, [&](int i) {
        const size_t o = (size_t)i * PB + t.un;
        return (hs == -2) ? __int_as_float(0x7fc00000) : ((i <= hs) ? fmaf(g, fsr[o], xs[o]) : 0.0f);
    });
}

hipError_t launch_ellip_kern(hipStream_t s, const EllipKernArgs &a, const EllipTransposeArgs &t)
{
    const size_t total = (size_t)a.B * a.P;
    hipLaunchKernelGGL(surfdisp_ellip_kern_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(surfdisp_ellip_transpose_kernel, rows_grid(t.B, t.P, t.Lmax, 3u), dim3(256), 0, s, t);
    return hipGetLastError();
}

}  // namespace sd


#ifdef SD_COUNT_RESTARTS
// development build only: read (and with reset != 0 clear) the restart counts {lanes, wavefronts}
extern "C" int surfdisp_dev_restart_count(unsigned long long *out2, int reset)
{
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpyFromSymbol(out2, HIP_SYMBOL(sd::sd_restart_count), 2 * sizeof(unsigned long long));
    if (e == hipSuccess && reset) {
        const unsigned long long z[2] = {0, 0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(sd::sd_restart_count), z, sizeof(z));
    }
    return (int)e;
}
#endif
