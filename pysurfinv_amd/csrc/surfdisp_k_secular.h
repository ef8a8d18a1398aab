#pragma once
// surfdisp_k_secular.h -- the secular functions of surfdisp_kernels.hip, state in registers: the LDS working-stack layout,
// the fp32 helpers, layer_coef, ray_* / delta_rayleigh*, delta_love*, the reference restatements, drop_layers, pair_swap.
#include "surfdisp_internal.h"
#include "surfdisp_k_common.h"

namespace sd {

// ================================================================ secular functions (registers)
// LDS working stack of one team: w[m*LS + f*S + slot], f = 0..5 (derived slot W_IR, b, rho, d, 1/a^2, 1/b^2):
// the six values of a layer sit at compile-time offsets f*S from one address (ds_read immediates)
constexpr int NFW = 6;
// Layer stride LS (words) for S = SD_PHASE_BLOCK / G slots: NFW * S padded so that the lanes of a team - which take
// consecutive LAYERS when they (re)build the stack, snapshot it or sum its thicknesses - fall into different LDS banks
// together with the neighbouring teams of their 32-lane group.  NFW * S is a multiple of 32 words for every team size
// up to 16 lanes: unpadded, all lanes of a team hit ONE bank (16-way conflicts on each of the 36 writes of a rebuild;
// SQ_LDS_BANK_CONFLICT was 29-55 % of the LDS cycles, profiles/r03a).  Wanted: lane j, neighbouring slot t -> bank
// (j * LS + t) mod 32 all different, i.e. LS = q * odd (mod 32) with q = 32 / G slots per group (1 for G >= 32).
// Love needs four of the six fields (1/(rho b^2), b, rho, d: 1/b^2 = 1/(rho b^2) x rho is one multiplication in the
// recursion): its working stacks take two thirds of the LDS - what decides how many Love workgroups fit beside the
// Rayleigh ones of a joint solve.
constexpr int NFW_LOVE = 4;
SD_HD constexpr int lds_ls(int S, int NF = NFW)
{
    const int G = SD_PHASE_BLOCK / S;
    const int q = (G >= 32) ? 1 : 32 / G;
    int ls = NF * S;
    while (ls % (2 * q) != q) ++ls;
    return ls;
}
// LS: the layer stride of the working stack at hand (a variable or parameter of the code that uses the macros)
#define W_AT(m, f) wq[(m) * LS + (f) * S]
#define W_IR(m) W_AT(m, 0)    // Rayleigh: layer 0 1/rho, layer m >= 1 rho(m-1)/rho(m) (rescale factor of the carried state); Love: 1/(rho b^2)
#define W_B(m) W_AT(m, 1)
#define W_R(m) W_AT(m, 2)
#define W_D(m) W_AT(m, 3)
#define W_IA2(m) W_AT(m, 4)   // 1/a^2  (c-independent; saves a division per layer per trial)
#define W_IB2(m) W_AT(m, 5)   // 1/b^2  (0 for a liquid layer)

// ---- fast-but-tight fp32 helpers for the inner recursion --------------------------------------
// The reference evaluates ~9 IEEE divisions, 2 sqrt and 2-4 libm calls per layer per trial
// velocity.  Here: reciprocal = v_rcp_f32 + one Newton step (<= 1 ulp), sqrt = v_sqrt_f32 (1 ulp),
// sinh/cosh = two v_exp_f32 (~1 ulp), sincos = 3-constant Cody-Waite reduction + minimax
// polynomials (~1 ulp for |x| < 1e4).  Every one of these perturbs a matrix entry by ~1e-7
// relative, i.e. like a 1e-7 relative change of a layer's thickness or velocity -- physically
// nothing; measured end-to-end parity is unchanged.
__device__ __forceinline__ float rcp_nr(float x)
{
    float r = __builtin_amdgcn_rcpf(x);
    return fmaf(r, fmaf(-x, r, 1.0f), r);
}
__device__ __forceinline__ float sqrt_hw(float x) { return __builtin_amdgcn_sqrtf(x); }
// v_rsq_f32 and v_exp_f32.  The host versions only let a CPU test compile layer_coef (tests/hostcheck/lcoefcheck.hip).
SD_HD __forceinline__ float rsq_hw(float x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_rsqf(x);
#else
    return 1.0f / sqrtf(x);
#endif
}
SD_HD __forceinline__ float exp2_hw(float x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_exp2f(x);
#else
    return exp2f(x);
#endif
}
// sinh(x), cosh(x): 0.5 e^x and 0.5 e^-x straight from v_exp_f32 (the 0.5 folded into the exponent)
SD_HD __forceinline__ void sinhcosh_sp(float x, float *sh, float *ch)
{
    // no low-order correction of x log2(e): e^x and e^-x then carry relative errors +-|x| 9e-8, which for |x| > 1 is a
    // common scale factor of sinh and cosh (the secular function's root does not move) - root search 6 % faster
    // (profiles/r02d/ab_recursion_variants.txt).  For |x| < 1 that is below one ulp of cosh, NOT of sinh: p - q has an
    // ABSOLUTE error of ~6e-8 for every x, a relative one of 6e-8 / |x| - callers that need sinh of small arguments
    // (layer_coef) replace it by a series there.
    // Tried and dropped (r02e): the pair scaled by e^-|x| from ONE exponential ((1 +- e^-2|x|)/2; a transcendental costs
    // four plain instructions).  The secular function then comes out times s(c) = exp(-sum |x|): same roots and signs,
    // but s has a square-root kink wherever c crosses a layer velocity and bends the function between them, and the
    // refine step interpolates - the unscaled function is what the reference's NEVILL sees.  Measured: 4.7 % faster, c
    // against the exact kernel 5.4e-6 -> 1.2e-5, one sediment fixture entry 5.5e-5; made safe (kink test, unscaled
    // values for NEVILL, overflow cue from the product of the factors) the gain was gone (profiles/r02e/ab_experiments.txt).
    const float t = x * 1.44269502e+00f;
    const float p = exp2_hw(t - 1.0f), q = exp2_hw(-t - 1.0f);
    *sh = p - q;
    *ch = p + q;
}
// The quadrant n picks sin or cos of the reduced argument (one compare, two selects) and flips their signs by an XOR of the
// sign bit: sin for n = 2, 3 (mod 4), cos for n = 1, 2.  Odd in x to the bit for every x != 0 (rint, the reduction and ps
// are odd, pc even, and n -> -n swaps the signs as sin and cos do) - layer_coef relies on it.
SD_HD __forceinline__ void sincos_cw(float x, float *sn, float *cs)
{
    const float TWO_OVER_PI = 6.36619747e-01f;
    const float P1 = 1.57079601e+00f, P2 = 3.13916473e-07f, P3 = 5.39030253e-15f;   // pi/2 split (Cody-Waite)
    const float q = __builtin_rintf(x * TWO_OVER_PI);
    float r = fmaf(-q, P1, x);
    r = fmaf(-q, P2, r);
    r = fmaf(-q, P3, r);
    const int n = (int)q;
    const float r2 = r * r;
    // minimax on [-pi/4, pi/4] (Cephes sinf/cosf coefficients)
    float ps = fmaf(fmaf(fmaf(-1.9515295891e-4f, r2, 8.3321608736e-3f), r2, -1.6666654611e-1f), r2 * r, r);
    float pc = fmaf(fmaf(fmaf(2.443315711809948e-5f, r2, -1.388731625493765e-3f), r2, 4.166664568298827e-2f),
                    r2 * r2, fmaf(-0.5f, r2, 1.0f));
    const float s0 = (n & 1) ? pc : ps;
    const float c0 = (n & 1) ? ps : pc;
    *sn = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s0) ^ ((uint32_t)(n & 2) << 30));
    *cs = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, c0) ^ ((uint32_t)((n + 1) & 2) << 30));
}

// The working stack's derived per-layer values (W_IR, W_IA2, W_IB2), one expression each, shared by the root search's
// rebuild (build in phase_body), the ellipticity kernel's replay and the tests' device probe (tests/probe): v_rcp + one
// Newton step (<= 1 ulp) instead of the reference's IEEE divisions.
__device__ __forceinline__ float wk_ia2(const float a) { return rcp_nr(a * a); }                          // 1/a^2
__device__ __forceinline__ float wk_ib2(const float b) { return (b > 0.0f) ? rcp_nr(b * b) : 0.0f; }    // 1/b^2, 0 if liquid
__device__ __forceinline__ float wk_irho(const float rho) { return rcp_nr(rho); }                        // Rayleigh layer 0: 1/rho
__device__ __forceinline__ float wk_rat(const float rho_prev, const float rho) { return rho_prev * rcp_nr(rho); }   // layer m >= 1
__device__ __forceinline__ float wk_ilove(const float rho, const float b) { return rcp_nr(rho * b * b); }  // Love: 1/(rho b^2)

// One wave type's coefficients in one layer, shared by ray_step (P, S and the liquid top layer), delta_love and - through
// ray_step - the ellipticity passes.  arg = 1 - c^2/v^2 (> 0: evanescent), wd = k d; r = sqrt(-arg) continued to
// r = -sqrt(arg) on the evanescent side, x = wd r:
//      rsin = r sin x,  sinr = sin(x) / r,  cs = cos x        (sinh / cosh on the evanescent side: rsin = -r sinh x,
//      ph = x where oscillatory, else 0                         sinr = sinh(x) / r, cs = cosh x, surfa.f:263-279)
// |arg| is clamped away from zero: c == v to the last bit then runs through the oscillatory formulas with r = 1e-15, which
// give the degenerate values (rsin = 0, sinr = k d, cs = 1) to 1e-15 - no separate branch.
// r = copysign(|r|, -arg), but each branch takes the sign from what it knows rather than from a bit-insert before the branch:
// evanescent, r < 0 and the negations ride on the products as source modifiers; oscillatory, r > 0 except at arg = +0 (and
// a NaN with a clear sign bit), and rsin, sinr and cs are even in r (sincos_cw is odd), so they are evaluated at k d |r| and
// only r, x and ph - which the default root search does not use - pay for the sign.  Bit for bit the values of the form
// with r signed before the branch wherever k d |r| != 0 (tests/test_layer_coef_bits.py); k d |r| = 0 needs a layer of zero
// thickness, which the prep kernel rejects.
struct LCoef { float r, rsin, sinr, cs, x, ph; };
template <bool SKIP = true>
SD_HD __forceinline__ LCoef layer_coef(const float arg, const float wd)
{
    const float xs = fmaxf(fabsf(arg), 1.0e-30f), y = rsq_hw(xs);
    const float ra = xs * y;                                    // |r| = x rsq(x) to ~1.5 ulp
    LCoef o;
    if (arg > 0.0f) {
        o.r = -ra;
        o.x = wd * o.r;
        float sh, ch; sinhcosh_sp(o.x, &sh, &ch);
        // sinh of a small argument: the difference of the two exponentials carries their absolute error (~6e-8), i.e. a
        // relative error 6e-8 / |x| that sinr = sinh(x) / r passes on - 1 % one float below a thin layer's velocity, a jump
        // of the secular function where c crosses it.  Below |x| = 1/4 the odd series to x^5 (truncation < 5e-8 relative;
        // above, the exponentials' error is < 4e-7 relative).  Cost: 4-6 % of the root search, 5.6 % of the headline, when
        // every lane evaluates it.  SKIP (device): the series and its select run only where some active lane of the
        // wavefront takes them (one compare into vcc, one scalar branch; the lanes that take them see the same
        // expressions, so every lane's value is the bits it was).  On the bench stacks a P coefficient needs the series
        // in under 2 % of the lane slots and a wavefront of 64 stacks in a quarter of its S coefficients: root search of
        // four-lane teams 1.364 -> 1.312 ms (-3.8 %), 993 -> 931 M wave-level VALU instructions per launch (-6.3 %),
        // 16-lane teams of 96-layer stacks 5.2 -> 4.9 ms (profiles/r10a).  Not for 64-lane teams (SKIP = false, phase_body):
        // the lanes of a wavefront are then 64 trial velocities of ONE stack, some lane nearly always needs the series,
        // and the branch only splits the block the scheduler hides the exponentials' latency in - the Metropolis lock
        // step of 1 500 x 96-layer stacks 1.43 -> 1.48 ms with it.  32-lane teams were not measured: off.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(SD_NO_SINH_SKIP)
        if (!SKIP || __builtin_amdgcn_ballot_w64(fabsf(o.x) < 0.25f) != 0ull)
#endif
        {
            const float x2 = o.x * o.x;
            const float shs = fmaf(o.x * x2, fmaf(x2, 8.33333333e-3f, 1.66666667e-1f), o.x);
            if (fabsf(o.x) < 0.25f) sh = shs;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(SD_NO_SINH_SKIP)
            // (an empty statement the compiler may not move: without it the five instructions are hoisted above the
            // branch again and every wavefront pays for them)
            if (SKIP) asm volatile("" : "+v"(sh));
#endif
        }
        o.rsin = ra * sh; o.sinr = sh * -y; o.cs = ch;
        o.ph = 0.0f;
    } else {
        o.r = copysignf(ra, -arg);
        o.x = wd * o.r;
        float sn, cs; sincos_cw(wd * ra, &sn, &cs);
        o.rsin = ra * sn; o.sinr = sn * y; o.cs = cs;
        o.ph = o.x;
    }
    return o;
}

// Rayleigh, production kernel: Dunkin's compound-matrix recursion (surfa.f:193-357) in a form built for the VALU.
// start = 1 -> dispersion (returns -bb1, surfa.f:357); start = 2 / 3 -> the two ellipticity passes (bb1, surfa.f:360-363).
//
// The layer's compound matrix is never formed.  Its fifteen entries (surfa.f:289-320) are linear in the nine products
// (cosp, rsinp, sinpr) x (cosq, rsinq, sinqr); collecting the update by product instead of by entry gives, exactly
// (algebraic identity, checked in fp64 to 3e-14; same fp32 error against an fp64 evaluation as the entry-by-entry form),
//   h = (b2, b3, b4)/rhoc, h5 = b5/rhoc^2,  u1 = g^2 b1 + 2g h3 - h5,  u2 = g1^2 b1 + 2g1 h3 - h5,
//   E1 = rsinp (rsinq u1 + cosq h2) - cosp rsinq h4 + (1 - cosp cosq) u2,
//   E2 = sinpr (sinqr u2 - cosq h4) + cosp sinqr h2 + (1 - cosp cosq) u1,
//   b1' = b1 - E1 - E2,  h3' = h3 + g E1 + g1 E2,  h5' = h5 + g^2 E1 + g1^2 E2,
//   h2' = cosp (cosq h2 + rsinq u1) + sinpr (rsinq h4 + cosq u2),
//   h4' = rsinp (sinqr h2 - cosq u1) - cosp (sinqr u2 - cosq h4).
// The state is carried as (b1, h2..h5): going from layer m to m+1 only rescales it by rho_m/rho_(m+1) (rhoc = rho c^2
// and c is the same), and the half-space row is applied to rhoc h.  ~40 operations per layer instead of ~100.
// Vertical wavenumbers ra, rb and their reciprocals come from ONE v_rsq_f32 each; sinh/cosh from two v_exp_f32.
// (The reference's own arithmetic, statement by statement, is delta_rayleigh_ref below: the exact fallback kernel.)
// One trial velocity's constants, the carried state and a layer's five values (rat: rho(m-1)/rho(m), formed when the
// working stack is built).  ray_step / ray_close are shared by the root search (delta_rayleigh: layer values from the LDS
// working stack) and by the ellipticity kernel (surfdisp_ellip_kernel: layer values rebuilt in registers) - the same
// expressions, so a (c, stack state) pair gives the same value whichever kernel evaluates it.
struct RTrial { float wvno, csq, icsq; };
struct RState { float b1, h2, h3, h4, h5; };
struct RLyr { float sv, d, ia2, ib2, rat; };
__device__ __forceinline__ RTrial ray_trial(const float c, const float T)
{
    RTrial t;
    t.wvno = 6.28318531f * rcp_nr(c * T);                 // <= 1 ulp: like a 6e-8 change of the period
    t.csq = c * c;
    t.icsq = rcp_nr(t.csq);
    return t;
}
// start vector (1,0,0,0,0) / e2 / e3 in the scale of the top layer (irho0 = 1 / rho of layer 0)
__device__ __forceinline__ RState ray_start(const RTrial &t, const int start, const float irho0)
{
    const float irhoc0 = (start == 1) ? 0.0f : irho0 * t.icsq;
    return RState{(start == 1) ? 1.0f : 0.0f, (start == 2) ? irhoc0 : 0.0f, (start == 3) ? irhoc0 : 0.0f, 0.0f, 0.0f};
}
// FIRST: only the TOP layer may be liquid in the production kernel (a stack with a liquid layer further down is handed
// to the exact fallback kernel by the prep kernel's statistics), so the test is made once per evaluation
// CERT (r04, the COUNT-GUIDED coarse scan for Rayleigh - the opt-in SURFDISP_FASTSCAN; the default scan walks every grid point):
// the state's first component b1 is det U_s of the two solutions that satisfy the free-surface condition (start: U = I, tractions
// 0).  At a trial (k, omega) the number of mode branches below it is
//      N = #{zeros of det U_s(z) over the stack} + #{positive eigenvalues of Z_h - Z_s at the top of the half space}
// (Morse index of the Neumann problem + the half space's boundary index; Z = T U^-1 with the tractions ordered (tr, tz), which
// makes the motion-stress system Hamiltonian and Z symmetric).  The zeros are counted LAYER BY LAYER, inside each layer, by
// Wittrick and Williams' rule (below) - exact in exact arithmetic while every oscillatory layer's S phase stays below pi
// (scripts/analysis/rayleigh_count_ww*.py: equal to the brute-force count on every such trial of 50 random stacks).  The first
// attempt looked at the sign of b1 at the interfaces only and missed pairs of zeros inside one layer
// (profiles/r04a/rayleigh_count.txt: 25 of 1.3e8 soak stacks on another root).
// What the count is NOT: a proof that an interval between two trials with equal counts holds no root.  Along the scan's line
// omega = const the count rises where the line crosses a branch whose group velocity is positive and FALLS where it is negative:
// a branch with a zero-group-velocity point (soft sediments with Vp/Vs near 3 over rock) can be crossed twice between two coarse
// points, +1 then -1.  Love branches cannot (their group velocity is an energy ratio of one sign; the Love certificate is a
// theorem); Rayleigh ones can, and two soak stacks in 1.2e9 did (profiles/r04b/rayleigh_count_ww.txt).  Hence opt-in.
// kc accumulates the count, kunc flags a trial whose count is not safe (a sign within rounding, an S phase beyond the bound, a
// liquid layer).
#ifndef SD_RCERT_SPHASE
#define SD_RCERT_SPHASE 3.0f    // S phase (rad) of an oscillatory layer up to which its in-layer count is taken (the theorem's bound: pi)
#endif
// mid(0) and mid(1): called once the step has read all of the layer's values and again after the P coefficients - where the
// single-register-set loop of delta_rayleigh issues the next layer's loads into the registers the step has freed (not
// called by a liquid top layer)
struct NoMid { __device__ void operator()(int) const {} };
template <bool FIRST, bool CERT = false, bool SKIP = true, class Mid = NoMid>
__device__ __forceinline__ void ray_step(RState &s, const RTrial &t, const RLyr &y, const int start, float &phi, int *kc = nullptr,
                                         bool *kunc = nullptr, const Mid &mid = Mid())
{
    float b1 = s.b1, h2 = s.h2, h3 = s.h3, h4 = s.h4, h5 = s.h5;
    const float wvno = t.wvno, csq = t.csq, icsq = t.icsq;
    const float sv = y.sv, d = y.d, ia2 = y.ia2, ib2 = y.ib2;
    if (!FIRST) {                                      // into this layer's scale: rhoc_prev / rhoc = rho_prev / rho
        const float rat = y.rat;
        h2 *= rat; h3 *= rat; h4 *= rat; h5 *= rat * rat;
    }
    const float arga = fmaf(-csq, ia2, 1.0f);                    // 1 - c^2/a^2, surfa.f:211
    const float wd = wvno * d;
    if (FIRST && !(fabsf(sv) > ACCUR)) {
        // liquid surface layer, surfa.f:216-251 (skipped entirely in the ellipticity passes): only a11 = cosp and
        // a21 = rhoc sinpr are non-zero (surfa.f:236-250)
        if (start != 1) return;
        if (CERT) *kunc = true;                            // (a liquid layer: no certificate)
        const LCoef P = layer_coef<SKIP>(arga, wd);
        const float sinpr = P.sinr, cosp = P.cs;
        phi += P.ph;
        const float n1 = cosp * b1;
        const float n2 = sinpr * b1;
        const float n5 = cosp * h5 - sinpr * h4;
        s.b1 = n1; s.h2 = n2; s.h3 = 0.0f; s.h4 = 0.0f; s.h5 = n5;
        return;
    }
    mid(0);
    const float argb = fmaf(-csq, ib2, 1.0f);
    const float g = 2.0f * (sv * sv) * icsq;
    const float g1 = g - 1.0f;
    const LCoef P = layer_coef<SKIP>(arga, wd);                              // surfa.f:263-279
    mid(1);
    const LCoef Q = layer_coef<SKIP>(argb, wd);
    const float rsinp = P.rsin, sinpr = P.sinr, cosp = P.cs;
    const float rsinq = Q.rsin, sinqr = Q.sinr, cosq = Q.cs, qm = Q.x;
    phi += P.ph;
    phi += Q.ph;
    const float g2 = g * g, g12 = g1 * g1;
    const float u1 = fmaf(g2, b1, fmaf(g + g, h3, -h5));
    const float u2 = fmaf(g12, b1, fmaf(g1 + g1, h3, -h5));
    const float D = fmaf(-cosp, cosq, 1.0f);
    const float t1 = fmaf(rsinq, u1, cosq * h2);            // rsinq u1 + cosq h2
    const float t2 = fmaf(sinqr, u2, -(cosq * h4));         // sinqr u2 - cosq h4
    const float Cx = cosp * rsinq, Cy = cosp * sinqr;
    const float E1 = fmaf(rsinp, t1, fmaf(-Cx, h4, D * u2));
    const float E2 = fmaf(sinpr, t2, fmaf(Cy, h2, D * u1));
    const float n1 = (b1 - E1) - E2;
    if (CERT) {
        // Zeros of det U_s INSIDE this layer (Wittrick-Williams).  With the surface pair's impedance Z_t at the layer's top and the
        // layer's propagator in blocks, det U_s at depth z below the top vanishes where M(z) = Z_t - K11(z) is singular, K11 = the
        // impedance of the slab clamped at z seen from its top; M(0+) is positive definite and - as long as no clamped-clamped
        // mode of the slab lies below the frequency, which Korn's inequality guarantees while the S phase k d r_beta < pi (and
        // always where S is evanescent) - its eigenvalues only move down: the zeros inside the layer = the negative eigenvalues
        // of M(d), 0, 1 or 2.  n1 is linear in the state, n1 = c1 b1 + c2 h2 + c3 h3 + c4 h4 + c5 h5, and for a state that is the
        // minors of [I; Z] (b1 = 1, h2 = -z22, h3 = -z12, h4 = z11, h5 = det Z) that is c5 det(Z - K11): K11's entries are ratios
        // of the coefficients, and
        //      det M = n1 / (b1 c5),      M11 = (h4 c5 - c2 b1) / (b1 c5),
        //      c5 = rsinp rsinq + sinpr sinqr + 2 (1 - cosp cosq),   c2 = -(rsinp cosq + cosp sinqr)
        // (scripts/analysis/rayleigh_count_ww*.py: per layer and in total equal to the finely stepped / brute-force counts on
        // every trial with all S phases below pi).  Unsafe: an oscillatory layer beyond SD_RCERT_SPHASE, or any of the three
        // signs within rounding (n1, c5, and - where it decides - M11's numerator against their own terms).
        const float p1 = rsinp * rsinq, p2 = sinpr * sinqr;
        const float c5 = p1 + p2 + (D + D);
        const float c2 = -fmaf(rsinp, cosq, Cy);
        const float bc = b1 * c5;
        const float m11a = h4 * c5, m11b = c2 * b1;
        const float m11n = m11a - m11b;
        const bool dneg = (n1 < 0.0f) != (bc < 0.0f);
        const bool mneg = (m11n < 0.0f) != (bc < 0.0f);
        *kc += dneg ? 1 : (mneg ? 2 : 0);
        *kunc = *kunc || (!(argb > 0.0f) && !(fabsf(qm) < SD_RCERT_SPHASE)) ||
                !(fabsf(n1) > 1.0e-4f * (fabsf(b1) + fabsf(E1) + fabsf(E2))) ||
                !(fabsf(c5) > 1.0e-4f * (fabsf(p1) + fabsf(p2) + 2.0f * fabsf(D))) ||
                (!dneg && !(fabsf(m11n) > 1.0e-4f * (fabsf(m11a) + fabsf(m11b)))) || !(fabsf(bc) > 0.0f);
    }
    const float n3 = fmaf(g, E1, fmaf(g1, E2, h3));
    const float n5 = fmaf(g2, E1, fmaf(g12, E2, h5));
    const float n2 = fmaf(cosp, t1, sinpr * fmaf(rsinq, h4, cosq * u2));
    const float n4 = fmaf(rsinp, fmaf(sinqr, h2, -(cosq * u1)), -(cosp * t2));
    s.b1 = n1; s.h2 = n2; s.h3 = n3; s.h4 = n4; s.h5 = n5;
}
// half-space closure, surfa.f:340-354, on (b1, rhoc h2..h4, rhoc^2 h5) with rhoc of the last layer gone through
// (a itself is not needed: every occurrence is a^2, available as 1/ia2); A = the values of layer mmax - 1, rho_last its
// density, rho_prev the density of layer mmax - 2 (0 when there is none: the state is in that layer's scale)
// *mag (if given): the sum of the magnitudes of the closure's five terms - |value| far below it means the value is the
// remainder of a cancellation, i.e. its SIGN is within the rounding of this arithmetic (the ellipticity passes' test)
__device__ __forceinline__ float ray_close(const RState &s, const RTrial &t, const RLyr &A, const float rho_last,
                                           const float rho_prev, const int start, float *mag = nullptr, const bool want_mag = true,
                                           int *kc = nullptr, bool *kunc = nullptr)
{
    const float csq = t.csq, icsq = t.icsq;
    const float sv = A.sv, ia2 = A.ia2;
    const float irho = rcp_nr(rho_last);
    const float rhoc = rho_prev * csq;
    const float arga = fmaf(-csq, ia2, 1.0f);
    float ra = sqrt_hw(fabsf(arga));
    if (arga > 0.0f) ra = -ra;
    const float argb = fmaf(-csq, A.ib2, 1.0f);
    float rb = sqrt_hw(fabsf(argb));
    if (argb > 0.0f) rb = -rb;
    const float sss = sv * sv;
    const float g = 2.0f * sss * icsq;
    const float g1 = g - 1.0f;
    const float gra = g * ra, g1s = g1 * g1;
    const float ira = rcp_nr(ra), igra = rcp_nr(gra), ig = rcp_nr(g);
    const float it12 = ia2 * irho;                                   // 1/(rho a^2)
    const float rba = rb - ira;
    const float h11 = -2.0f * rb * sss * ia2 + csq * g1s * ia2 * igra;
    const float h13 = -rb * it12 + g1 * it12 * igra;
    const float h14 = rb * it12 * igra;
    const float h15 = rba * (irho * irho) * ia2 * icsq * ig;         // rba/(rho a)^2/c^2/g
    const float h12 = -ig * it12;
    const float bb1 = h11 * s.b1 + rhoc * (h12 * s.h2 + 2.0f * h13 * s.h3 + h14 * s.h4 + rhoc * (h15 * s.h5));
    if (kc) {
        // boundary index at the top of the half space: positive eigenvalues of S = Z_h - Z_s (both divided by k > 0),
        //   Z_s = (rhoc / b1) [[h4, -h3], [-h3, -h2]]   (b2..b4 = -minors / k: rhoc h2..h4 of this state),
        //   Z_h = rho c^2 / (1 - ra rb) [[-ra, g1 - g ra rb], [g1 - g ra rb, -rb]]   (ra, rb > 0: the half space's decaying pair)
        const float rap = fabsf(ra), rbp = fabsf(rb);
        const float zf = rho_last * csq * rcp_nr(1.0f - rap * rbp), zo = g1 - g * rap * rbp;
        const float sf = rhoc * rcp_nr(s.b1);
        const float S11 = -zf * rap - sf * s.h4, S12 = zf * zo + sf * s.h3, S22 = -zf * rbp + sf * s.h2;
        const float dq = S11 * S22 - S12 * S12, tp = S11 + S22;
        *kc += (dq < 0.0f) ? 1 : ((tp > 0.0f) ? 2 : 0);
        // unsafe: the half space not evanescent in P and S, a determinant or - where it matters - a trace within rounding, not finite
        *kunc = *kunc || !(arga > 0.0f) || !(argb > 0.0f) || !(fabsf(dq) > 1.0e-4f * (fabsf(S11 * S22) + S12 * S12)) ||
                (dq > 0.0f && !(fabsf(tp) > 1.0e-4f * (fabsf(S11) + fabsf(S22)))) || !fin(dq) || !fin(s.b1) || s.b1 == 0.0f;
    }
    if (mag && want_mag) *mag = fabsf(h11 * s.b1) + fabsf(rhoc) * (fabsf(h12 * s.h2) + 2.0f * fabsf(h13 * s.h3) + fabsf(h14 * s.h4) +
                                                        fabsf(rhoc * (h15 * s.h5)));
    return (start == 1) ? -bb1 : bb1;
}

// *bhs (if given) receives the half space's b - A.sv of layer mmax - 1, the LDS word the scan's upper guard compares the
// trial with (see LEAN_BHS in phase_body)
template <bool PIPE2 = true, bool CERT = false, bool SKIP = true>
__device__ __forceinline__ float delta_rayleigh(const float *wq, const int LS, const int S,
                                                const int mmax, const float c, const float T,
                                                const int start, float &phi, float *mag = nullptr, const bool want_mag = true,
                                                int *kcp = nullptr, bool *kuncp = nullptr, const bool count = false,
                                                float *bhs = nullptr
#ifdef SD_WAVECLOCK
                                                , unsigned long long *wsec = nullptr   // cycles: [0] head, [1] layer loop, [2] closure
#endif
                                                )
{
#ifdef SD_WAVECLOCK
    const unsigned long long ws0 = __builtin_readcyclecounter();
#endif
    int kc_ = 0; bool kunc_ = !count;
    int *const kc = &kc_; bool *const kunc = &kunc_;
    // phi: vertical phase sum_i k d_i sqrt(c^2/v_i^2 - 1) over the layers (and wave types) that are oscillatory
    // at c -- the WKB mode counter (free: pm and qm are the recursion's own arguments; read by tests/probe only since the
    // r01 scan that bounded it between two coarse points is gone)
    phi = 0.0f;
    const RTrial t = ray_trial(c, T);
    RState s = ray_start(t, start, (start == 1) ? 0.0f : W_IR(0));
    // software pipeline: layer m+1's LDS values are in flight while layer m is computed.  The loop
    // is unrolled by two over alternating register sets (no rotation moves between iterations).
    auto load = [&](int m) -> RLyr { return {W_B(m), W_D(m), W_IA2(m), W_IB2(m), W_IR(m)}; };
    const int last = mmax - 1;                                       // the half space
    RLyr A = load(0);
    int m = 0;
#ifdef SD_WAVECLOCK
    const unsigned long long ws1 = __builtin_readcyclecounter();   // (head: trial constants, start vector, first loads issued)
#endif
    if (last >= 1) {                                                 // layer 0: the one that may be water
        const RLyr Bq = load(1);
        if (CERT && count) ray_step<true, true, SKIP>(s, t, A, start, phi, kc, kunc); else ray_step<true, false, SKIP>(s, t, A, start, phi);
        A = Bq;
        m = 1;
    }
    if (PIPE2) {
        while (m + 2 <= last) {
            const RLyr Bq = load(m + 1);
            if (CERT && count) ray_step<false, true, SKIP>(s, t, A, start, phi, kc, kunc); else ray_step<false, false, SKIP>(s, t, A, start, phi);
            A = load(m + 2);
            if (CERT && count) ray_step<false, true, SKIP>(s, t, Bq, start, phi, kc, kunc); else ray_step<false, false, SKIP>(s, t, Bq, start, phi);
            m += 2;
        }
    } else {
        // (also the count-guided scan's instantiations: their extra scan state put teams of four at 133 VGPRs = three
        // wavefronts per SIMD, 27 M solves/s with one batch in flight; single-buffered 122 = four, 36 M.)
        // Teams of two lanes - what a caller with several batches in flight gets (SURFDISP_PIPELINED) - keep ONE register
        // set in flight: their wavefronts share SIMDs with the group-velocity kernel's (168 VGPRs), and three of them
        // fit beside one of those only while 3 x VGPRs + 168 <= 512 (101 this way; measured at 120: the three-batch
        // headline drops 7 %, profiles/r02e/ab_experiments.txt)
        // Layer m+1's values are loaded field by field once layer m's are no longer needed: d and 1/a^2 as soon as the step
        // has read the layer, 1/b^2 after the P coefficients, b and rho(m)/rho(m+1) after the update.  Each load is in flight
        // for a whole layer and lands in the registers of the field it replaces (loaded all at once at the top of the loop,
        // four values had to be copied at every layer).
        while (m + 1 <= last) {
            const int n = m + 1;
            auto mid = [&](int stage) {
                if (stage == 0) { A.d = W_D(n); A.ia2 = W_IA2(n); } else { A.ib2 = W_IB2(n); }
            };
            if (CERT && count) ray_step<false, true, SKIP>(s, t, A, start, phi, kc, kunc, mid); else ray_step<false, false, SKIP>(s, t, A, start, phi, nullptr, nullptr, mid);
            A.sv = W_B(n); A.rat = W_IR(n);
            m = n;
        }
    }
    if (m < last) {
        const RLyr Bq = load(m + 1);
        if (CERT && count) ray_step<false, true, SKIP>(s, t, A, start, phi, kc, kunc); else ray_step<false, false, SKIP>(s, t, A, start, phi);
        A = Bq;
    }
    // A holds layer mmax-1 here; the state is in the scale of the last layer stepped through
#ifdef SD_WAVECLOCK
    const unsigned long long ws2 = __builtin_readcyclecounter();
#endif
    const float v = ray_close(s, t, A, W_R(last), last >= 1 ? W_R(last - 1) : 0.0f, start, mag, want_mag,
                              (CERT && count) ? kc : nullptr, kunc);
    if (bhs) *bhs = A.sv;
    if (CERT) { *kcp = kc_; *kuncp = kunc_ || (last < 1); }
#ifdef SD_WAVECLOCK
    if (wsec) { wsec[0] += ws1 - ws0; wsec[1] += ws2 - ws1; wsec[2] += __builtin_readcyclecounter() - ws2; }
#endif
    return v;
}

// The exact fallback kernel's Rayleigh secular function: DLTAR4 restated statement by statement (surfa.f:193-357),
// IEEE division and square root, libm-grade exp / sin / cos, no fused multiply-adds - so that every intermediate
// overflows to inf, and every inf - inf turns NaN, exactly where the reference's does (which decides the "roots" the
// reference returns next to the overflowed region).  Working stack of that kernel: a in the W_IA2 slot.
// start = 1 -> dispersion (-bb1); 2 / 3 -> the two ellipticity passes (bb1), combined by the caller (surfa.f:360-363).
struct RefLyr { float a, b, rho, d; };
// GET: m -> the working stack's values of layer m (called for m = 0 .. mmax - 1, once each, in order)
template <class GET>
__device__ __forceinline__ float delta_rayleigh_ref_gen(GET get, const int mmax, const float c, const float t, const int start)
{
#pragma clang fp contract(off)
    const float accur = 1.e-8f, accurs = 1.e-8f;
    const float wvno = 6.28318531f / (c * t);
    const float csq = c * c;
    float b1 = (start == 1) ? 1.0f : 0.0f, b2 = (start == 2) ? 1.0f : 0.0f, b3 = (start == 3) ? 1.0f : 0.0f,
          b4 = 0.0f, b5 = 0.0f;
    float ra = 0.0f, rb = 0.0f, g = 0.0f, g1 = 0.0f;
    RefLyr yl{1.0f, 1.0f, 1.0f, 0.0f};
    for (int m = 0; m < mmax; ++m) {
        yl = get(m);
        const float pm_ = yl.a, sm = yl.b, rho = yl.rho, d = yl.d;             // p(m), s(m), rho(m), d(m)
        const float arga = 1.0f - csq / (pm_ * pm_);
        ra = sqrtf(fabsf(arga));
        if (arga > 0.0f) ra = -ra;
        float a11, a12, a13, a14, a15, a21, a22, a23, a24, a31, a32, a33, a41, a42, a51;
        if (!(fabsf(sm) > accurs)) {                       // liquid surface layer, surfa.f:216-251
            const float pm = wvno * ra * d;
            if (start > 1) continue;
            const float rhoc = rho * csq;
            float sinpr, cosp;
            if (fabsf(ra) < accur || ra == 0.0f) { sinpr = wvno * d; cosp = 1.0f; }
            else if (ra < 0.0f) { sinpr = (expf(pm) - expf(-pm)) / (2.0f * ra); cosp = 0.5f * (expf(pm) + expf(-pm)); }
            else { sinpr = sinf(pm) / ra; cosp = cosf(pm); }
            a11 = cosp; a21 = rhoc * sinpr;
            a31 = a41 = a51 = a12 = a22 = a32 = a42 = a13 = a23 = a33 = a14 = a24 = a15 = 0.0f;
        } else {
            const float argb = 1.0f - csq / (sm * sm);
            rb = sqrtf(fabsf(argb));
            if (argb > 0.0f) rb = -rb;
            g = 2.0f * (sm * sm) / csq;
            g1 = g - 1.0f;
            if (m == mmax - 1) break;                      // if(mmax-m) 40,52,40
            const float rhoc = rho * csq;
            const float pm = wvno * ra * d, qm = wvno * rb * d;
            float rsinp, sinpr, cosp, rsinq, sinqr, cosq;
            if (ra < 0.0f) { rsinp = -ra * 0.5f * (expf(pm) - expf(-pm)); sinpr = -rsinp / (ra * ra); cosp = 0.5f * (expf(pm) + expf(-pm)); }
            else if (ra == 0.0f) { rsinp = 0.0f; sinpr = wvno * d; cosp = 1.0f; }
            else { rsinp = ra * sinf(pm); sinpr = rsinp / (ra * ra); cosp = cosf(pm); }
            if (fabsf(rb) < accur) { rsinq = 0.0f; sinqr = wvno * d; cosq = 1.0f; }
            else if (rb > 0.0f) { rsinq = rb * sinf(qm); sinqr = rsinq / (rb * rb); cosq = cosf(qm); }
            else { rsinq = -rb * 0.5f * (expf(qm) - expf(-qm)); sinqr = -rsinq / (rb * rb); cosq = 0.5f * (expf(qm) + expf(-qm)); }
            const float rr = rsinp * rsinq, ss = sinpr * sinqr, cc = cosp * cosq;
            const float rs1 = rsinp * cosq, rs2 = sinqr * cosp, rs3 = sinpr * cosq, rs4 = rsinq * cosp;
            const float gm = 2.0f * g - 1.0f, gs = g * g, g1s = g1 * g1, ccm = 1.0f - cc, gg1 = g * g1;
            const float rhocs = rhoc * rhoc;
            const float suu = gs * rr + g1s * ss;
            a11 = 2.0f * gs - gm;
            a11 = a11 * cc - suu - 2.0f * gg1;
            a12 = -(rs1 + rs2) / rhoc;
            a13 = gm * ccm + g1 * ss + g * rr;
            a13 = -2.0f * a13 / rhoc;
            a14 = (rs3 + rs4) / rhoc;
            a15 = 2.0f * ccm + rr + ss;
            a15 = a15 / rhocs;
            a21 = rhoc * (g1s * rs3 + gs * rs4);
            a22 = cc;
            a23 = 2.0f * (g * rs4 + g1 * rs3);
            a24 = sinpr * rsinq;
            a31 = rhoc * (gg1 * gm * ccm + g1s * g1 * ss + gs * g * rr);
            a32 = g1 * rs2 + g * rs1;
            a33 = 1.0f + 2.0f * (2.0f * gg1 * ccm + suu);
            a41 = -rhoc * (g1s * rs2 + gs * rs1);
            a42 = rsinp * sinqr;
            a51 = rhocs * (2.0f * gs * g1s * ccm + gs * gs * rr + g1s * g1s * ss);
        }
        const float bb1 = a11 * b1 + a12 * b2 + a13 * b3 + a14 * b4 + a15 * b5;
        const float bb2 = a21 * b1 + a22 * b2 + a23 * b3 + a24 * b4 - a14 * b5;
        const float bb3 = a31 * b1 + a32 * b2 + a33 * b3 - 0.5f * a23 * b4 + 0.5f * a13 * b5;
        const float bb4 = a41 * b1 + a42 * b2 - 2.0f * a32 * b3 + a22 * b4 - a12 * b5;
        const float bb5 = a51 * b1 - a41 * b2 + 2.0f * a31 * b3 - a21 * b4 + a11 * b5;
        b1 = bb1; b2 = bb2; b3 = bb3; b4 = bb4; b5 = bb5;
    }
    // label 52: the half space (ra, rb, g, g1 of layer mmax from the last trip of the loop)
    const float pp = yl.a, sss = yl.b * yl.b, ppp = pp * pp;
    const float rhp = yl.rho * pp;
    const float gra = g * ra, g1s = g1 * g1, rba = rb - 1.0f / ra;
    const float h11 = -2.0f * rb * sss / ppp + csq * g1s / ppp / gra;
    float h12 = rhp * pp;
    const float h13 = -rb / h12 + g1 / h12 / gra;
    const float h14 = rb / h12 / gra;
    const float h15 = rba / rhp / rhp / csq / g;
    h12 = -1.0f / g / h12;
    const float bb1 = h11 * b1 + h12 * b2 + 2.0f * h13 * b3 + h14 * b4 + h15 * b5;
    return (start == 1) ? -bb1 : bb1;
}
__device__ __noinline__ float delta_rayleigh_ref(const float *wq, const int LS, const int S,
                                                 const int mmax, const float c, const float t, const int start)
{
    return delta_rayleigh_ref_gen([&](int m) { return RefLyr{W_IA2(m), W_B(m), W_R(m), W_D(m)}; }, mmax, c, t, start);
}

// Love: Thomson-Haskell 2-vector from the half space up, surfa.f:143-179 (production kernel; the reference's own
// arithmetic is delta_love_ref below).  Per layer: ONE v_rsq_f32 gives rb = sqrt|c^2/b^2 - 1| and 1/rb (|.| clamped away
// from zero: c == b then runs through the oscillatory formulas with rb = 1e-15, which give the reference's degenerate
// values y = -k d, z = 0, cosq = 1 of surfa.f:163-165 to 1e-15); 1/(rho b^2) comes from the working stack (the slot the
// Rayleigh recursion keeps its density ratios in).  Three transcendentals per evanescent layer instead of five.
// CERT: also the Sturm count of the trial - kc = net number of times the (displacement, stress) vector has crossed
// "stress = 0" clockwise on the way up from the half space (see the certified scan in phase_body), kunc = the count is not
// safe (a sign or a multiple of pi within rounding).  In a layer where c > b the pair (ut, tt / (h rb)) ROTATES by
// q = -k d rb: floor(|q| / pi) or one more crossings, the parity being whether tt changed sign; where c < b it moves along
// a hyperbola towards the diagonal and can cross at most once, counter-clockwise.
template <bool CERT = false, bool SKIP = true>
__device__ __forceinline__ float delta_love(const float *wq, const int LS, const int S,
                                            const int mmax, const float c, const float T, float &phi, int &kc, bool &kunc,
                                            const bool count = true, float *mag = nullptr)
{
    float lmag = 0.0f;                                     // |h z ut| + |cosq tt| of the last step (see ray_close's mag)
    kc = 0; kunc = !count;                                 // (count = false: no certificate from this trial)
    phi = 0.0f;                                            // see delta_rayleigh
    const float wvno = 6.2831853f * rcp_nr(c * T);
    const float csq = c * c;
    const int mh = mmax - 1;
    float bm = W_B(mh);
    float h = W_R(mh) * bm * bm;
    float rb = sqrt_hw(fabsf(fmaf(csq, W_IR(mh) * W_R(mh), -1.0f)));   // sqrt|c^2/b^2 - 1|, 1/b^2 = 1/(rho b^2) x rho
    float ut = 1.0f, tt = h * rb;
    // layer m-1's five LDS values are in flight while layer m is computed; unrolled by two over
    // alternating register sets
    struct Lyr { float b, d, r, ih; };
    auto load = [&](int m) -> Lyr { const int q = m > 0 ? m : 0; return {W_B(q), W_D(q), W_R(q), W_IR(q)}; };
    auto step = [&](const Lyr &y) {
        // contractions spelt out: every instantiation (certified scan, point-by-point scan, exact re-evaluation) must round
        // the same way - the certified scan's brackets are the point-by-point scan's only if the values agree to the bit
#pragma clang fp contract(off)
        bm = y.b;
        const float d = y.d, rho = y.r, ih = y.ih;
        if (bm == 0.0f) return;                            // water, surfa.f:152
        const float arg = fmaf(csq, ih * rho, -1.0f);      // c^2/b^2 - 1: < 0 evanescent
        h = rho * bm * bm;
        // the layer's coefficients at q = -k d rb: y = sin(q) / rb = -sinr, z = rb sin q = -rsin = -rb^2 y (rsin, sinr of
        // layer_coef at 1 - c^2/b^2 = -arg and +k d)
        const LCoef Q = layer_coef<SKIP>(-arg, wvno * d);
        rb = fabsf(Q.r);
        const float q = -Q.x;
        const float yv = -Q.sinr, z = -Q.rsin, cosq = Q.cs;
        phi -= (arg < 0.0f) ? 0.0f : q;
        const float eut = fmaf(cosq, ut, -(yv * tt * ih));
        const float ett = fmaf(h * z, ut, cosq * tt);
        lmag = fabsf(h * z * ut) + fabsf(cosq * tt);
        if (CERT && count) {
            const bool flip = (tt < 0.0f) != (ett < 0.0f);
            if (arg < 0.0f) {
                kc -= flip ? 1 : 0;
                // a pair that enters an evanescent layer close to its DECAYING direction (a mode trapped in a low-velocity
                // channel below a lid) leaves it as the difference of two e^{|q|} terms: below 1e-3 of them the sign of the
                // stress - here and in the point-by-point scan's secular function next to this trial - is rounding noise
                kunc = kunc || !(fabsf(ett) > 1.0e-3f * (fabsf(h * z * ut) + fabsf(cosq * tt)));
            } else {
                const float t = -q * 0.318309886f;         // |q| / pi
                const float nf = floorf(t), r = t - nf;
                const int nfull = (int)nf;
                kc += nfull + (((nfull & 1) != 0) != flip ? 1 : 0);
                kunc = kunc || (r > 1.0f - 4.0e-4f) || (nfull >= 1 && r < 4.0e-4f);      // |q| within ~1e-3 rad of a multiple of pi
            }
            kunc = kunc || !(fabsf(ett) > 1.0e-5f * (fabsf(ett) + fabsf(h * rb * eut)));  // stress ~ 0 at an interface (or not finite)
        }
        ut = eut; tt = ett;
    };
    int m = mh - 1;
    Lyr A = load(m);
    while (m >= 1) {
        const Lyr Bq = load(m - 1);
        step(A);
        A = load(m - 2);
        step(Bq);
        m -= 2;
    }
    if (m == 0) step(A);
    if (mag) *mag = lmag;
    return -tt;
}

// ... and its Love secular function: DLTAR1 statement by statement (surfa.f:143-179), same rules.
__device__ __forceinline__ float delta_love_ref_body(const float *wq, const int LS, const int S,
                                                     const int mmax, const float c, const float t)
{
#pragma clang fp contract(off)
    const float wvno = 6.2831853f / (c * t);
    float covb = c / W_B(mmax - 1);
    float h = W_R(mmax - 1) * W_B(mmax - 1) * W_B(mmax - 1);
    float rb = sqrtf(fabsf(covb * covb - 1.0f));
    float ut = 1.0f, tt = h * rb;
    for (int m = mmax - 2; m >= 0; --m) {
        const float bm = W_B(m);
        if (bm == 0.0f) continue;
        covb = c / bm;
        rb = sqrtf(fabsf(covb * covb - 1.0f));
        h = W_R(m) * bm * bm;
        const float d = W_D(m);
        const float q = -wvno * d * rb;
        float y, z, cosq;
        if (rb < 0.1e-20f || c - bm == 0.0f) { y = -wvno * d; z = 0.0f; cosq = 1.0f; }
        else if (c - bm < 0.0f) {
            const float exqp = expf(q), exqm = 1.0f / exqp;
            y = (exqp - exqm) / (2.0f * rb);
            z = -rb * rb * y;
            cosq = (exqp + exqm) / 2.0f;
        } else {
            const float sinq = sinf(q);
            y = sinq / rb; z = rb * sinq; cosq = cosf(q);
        }
        const float eut = cosq * ut - y * tt / h;
        const float ett = h * z * ut + cosq * tt;
        ut = eut; tt = ett;
    }
    return -tt;
}
__device__ __noinline__ float delta_love_ref(const float *wq, const int LS, const int S,
                                             const int mmax, const float c, const float t)
{
    return delta_love_ref_body(wq, LS, S, mmax, c, t);
}

// layer dropping for one trial velocity, surfa.f:94-105.  No early exit: every load is independent
// of the running sum, so the LDS reads pipeline instead of costing one round trip per layer
// (adding 0.0f for a skipped layer is exact, and nothing after the first crossing can change mm).
__device__ __forceinline__ int drop_layers(const float *wq, const int LS, const int S,
                                           const int n, const float c, const float T)
{
    // mmax = ii + 1 at the first layer ii whose running sum exceeds dmax.  The thicknesses are >= 0, so the running sums
    // never decrease and that layer is found by COUNTING the sums that do not exceed dmax: no "found" flag, no select
    // per layer (five vector instructions per layer and none on the scalar unit; the flag version took six + five)
    const float dmax = FACT * c * T;
    int cnt = 0;
    float sum = 0.0f;
#pragma unroll 8
    for (int ii = 0; ii < n; ++ii) {
        const float bi = W_B(ii), di = W_D(ii);
        sum = sum + ((c < bi) ? di : 0.0f);
        cnt += (sum > dmax) ? 0 : 1;
    }
    const int mm = (cnt < n) ? cnt + 1 : n;
    return mm < 2 ? 2 : mm;
}

// the other lane of a two-lane team (lane ^ 1): one DPP move (quad_perm [1,0,3,2]) instead of an LDS permute and its wait.
// Every lane of the wavefront must be active.
__device__ __forceinline__ int pair_swap(int x) { return __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ float pair_swap(float x) { return __int_as_float(pair_swap(__float_as_int(x))); }

}  // namespace sd
