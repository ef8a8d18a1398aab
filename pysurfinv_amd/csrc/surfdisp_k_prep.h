#pragma once
// surfdisp_k_prep.h -- K0 of surfdisp_kernels.hip: surfdisp_prep_kernel (validation, earth-flattening factors, the staged
// SoA / row copies of the model) and the layer read-out every later stage uses (LayerRaw, LayerV, layer_at).
#include "surfdisp_internal.h"
#include "surfdisp_k_common.h"

namespace sd {

// =================================================================================== K0: prep
// One lane per stack.  Flattening factors depend only on the radii, i.e. on the thickness prefix
// sums (flat1.f:33-37), not on the period or on how many layers are flattened:
//   regular layer i : dif_i, qqq_i (flat1.f:44-56), new thickness z1(i+1)-z1(i) (flat1.f:65-68)
//   layer i used as half space: hsf_i = a/r_i, hsr_i = (1/hsf_i)^pwr (flat1.f:58-62)
// The flattening factors difference nearly equal radii, which amplifies a 1-ulp difference between
// two powf/logf implementations to ~1e-3 of a thin layer's density/thickness.  Evaluate in fp64 and
// round once: that is the correctly rounded fp32 result, which is also what the reference's libm
// returns (glibc powf/logf are correctly rounded in all but vanishingly rare cases).
SD_HD __forceinline__ float powr32(float x, float y) { return (float)pow((double)x, (double)y); }
SD_HD __forceinline__ float log32(float x) { return (float)log((double)x); }

template <int KIND>
SD_HD inline void prep_stack(const PrepArgs &A, const int b)
{
    const int Lmax = A.Lmax, B = A.B;
    int n = A.nlay ? A.nlay[b] : Lmax;
    const float *src = A.model + (size_t)b * 5 * Lmax;
    float *mdl = A.mdl;
    bool ok = (n >= 2) && (n <= Lmax);
    const float pwr = pwr_of(KIND);
    const float apw = powr32(R0, pwr);
    float hmax = 0.0f, vs_prev = 0.0f, vp_prev = 0.0f;
    float hthick = 0.0f, rhomax = 0.0f, bmax = 0.0f;   // flattened: thickest layer, largest density and Vs
    bool mono = true;
    if (ok) {
        float hs = 0.0f;          // running thickness sum, fp32 in layer order (flat1.f:33-37)
        float r_i = R0;           // radius of the top of layer i
        float z_i = 0.0f;         // flattened depth of the top of layer i
        for (int i = 0; i < n; ++i) {
            const float vp = src[0 * Lmax + i], vs = src[1 * Lmax + i], rho = src[2 * Lmax + i];
            const float h = src[3 * Lmax + i], qs = src[4 * Lmax + i];
            if (!(fin(vp) && fin(vs) && fin(rho) && fin(h) && fin(qs)) ||
                !(vp > 0.0f) || !(rho > 0.0f) || (vs < 0.0f) || (h < 0.0f))
                ok = false;
            if (i < n - 1 && h > hmax) hmax = h;
            if ((i > 0 && (vs < vs_prev || vp < vp_prev))) mono = false;
            vs_prev = vs; vp_prev = vp;
            hs = hs + h;
            const float r_n = R0 - hs;                       // radius of the bottom of layer i
            float dif = 0.0f, qqq = 0.0f, dfl = 0.0f;
            if (i < n - 1) {
                const float fltd = log32(r_i / r_n);
                dif = (1.0f / r_n - 1.0f / r_i) * R0 / fltd;
                const float difr = powr32(r_i, pwr) - powr32(r_n, pwr);
                qqq = difr / (fltd * apw * pwr);
                const float z_n = R0 * log32(R0 / r_n);
                dfl = z_n - z_i;
                z_i = z_n;
                if (!(r_n > 0.0f) || !fin(dif) || !fin(qqq)) ok = false;
            }
            const float hsf = R0 / r_i;
            const float hsr = powr32(1.0f / hsf, pwr);
            // 6 % on the velocities for the attenuation correction (1 + qs ln(1/T)/pi, calcul.f:122-126)
            hthick = fmaxf(hthick, dfl);
            if (i > 0 && !(fabsf(vs) > ACCUR)) hthick = 1.0e30f;
            rhomax = fmaxf(rhomax, rho * fmaxf(qqq, hsr));
            bmax = fmaxf(bmax, 1.06f * vs * fmaxf(dif, hsf));
            const size_t o = (size_t)i * B + b;
            const size_t fs = (size_t)Lmax * B;
            const float v9[NF] = {vp, vs, rho, qs, dif, qqq, dfl, hsf, hsr};      // F_VP .. F_HSR
            for (int f = 0; f < NF; ++f) {
                if (A.write_soa) mdl[f * fs + o] = v9[f];
                if (A.rows) A.rows[((size_t)b * NF + f) * Lmax + i] = v9[f];
            }
            r_i = r_n;
        }
    }
    A.nl[b] = ok ? n : 0;          // 0 => BADMODEL: K1/K2 write zeros
    if (A.fsafe) A.fsafe[b] = (ok && mono) ? hmax : 1.0e30f;
    if (A.ovf) {                                               // inputs of the phase kernel's entry_overflow_risk
        A.ovf[b] = hthick;
        A.ovf[(size_t)B + b] = 2.0f * logf(fmaxf(rhomax, 1.0e-30f));
        A.ovf[2 * (size_t)B + b] = 4.0f * logf(fmaxf(2.0f * bmax * bmax, 1.0e-30f));
    }
    if (A.fb_count && b == 0) { A.fb_count[0] = 0; A.fb_count[1] = 0; A.fb_count[2] = 0; }   // empty list of stacks for the exact fallback; [1], [2]: scan trials / ellipticities re-evaluated
    if (A.nsolved_init) A.nsolved_init[b] = ok ? A.P : 0;      // independent mode: reduced with atomicMin
}

// Device version: TL lanes per stack (TL = 1 .. 64, a power of two), lane j owns layers j, j + TL, ...  The fp64
// pow / log of the flattening factors are most of the work and one lane walking 96 layers takes 0.22 ms whatever the
// batch size, so small batches spread a stack over a whole wavefront.  Bit-identical to prep_stack (which stays as the
// host reference of tests/hostcheck): the running thickness sum is formed in layer order by every lane for itself
// (fp32 adds only), and a layer's radii, depths and factors are the same expressions of that sum.
template <int KIND, int TL>
__global__ __launch_bounds__(256) void surfdisp_prep_kernel(PrepArgs A)
{
    const int Lmax = A.Lmax, B = A.B;
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = (int)(tid / TL), j = (int)(tid % TL);
    const bool valid = b < B;
    int n = valid ? (A.nlay ? A.nlay[b] : Lmax) : 0;
    const float *src = A.model + (size_t)(valid ? b : 0) * 5 * Lmax;
    float *mdl = A.mdl;
    bool ok = (n >= 2) && (n <= Lmax);
    if (!ok) n = 0;
    const float pwr = pwr_of(KIND);
    const float apw = powr32(R0, pwr);
    const size_t fs = (size_t)Lmax * B;
    float hmax = 0.0f, hthick = 0.0f, rhomax = 0.0f, bmax = 0.0f;
    bool mono = true;
    float hs = 0.0f;                // running thickness sum over layers < i0 (fp32, layer order: flat1.f:33-37)
    int i0 = 0;
    for (int i = j; i < n; i += TL) {
        for (; i0 < i; ++i0) hs = hs + src[3 * Lmax + i0];
        const float vp = src[0 * Lmax + i], vs = src[1 * Lmax + i], rho = src[2 * Lmax + i];
        const float h = src[3 * Lmax + i], qs = src[4 * Lmax + i];
        if (!(fin(vp) && fin(vs) && fin(rho) && fin(h) && fin(qs)) ||
            !(vp > 0.0f) || !(rho > 0.0f) || (vs < 0.0f) || (h < 0.0f))
            ok = false;
        if (i < n - 1 && h > hmax) hmax = h;
        if (i > 0 && (vs < src[1 * Lmax + i - 1] || vp < src[0 * Lmax + i - 1])) mono = false;
        const float r_i = R0 - hs;                           // radius of the top of layer i
        const float r_n = R0 - (hs + h);                     // ... and of its bottom
        const float z_i = (i == 0) ? 0.0f : R0 * log32(R0 / r_i);
        float dif = 0.0f, qqq = 0.0f, dfl = 0.0f;
        if (i < n - 1) {
            const float fltd = log32(r_i / r_n);
            dif = (1.0f / r_n - 1.0f / r_i) * R0 / fltd;
            const float difr = powr32(r_i, pwr) - powr32(r_n, pwr);
            qqq = difr / (fltd * apw * pwr);
            dfl = R0 * log32(R0 / r_n) - z_i;
            if (!(r_n > 0.0f) || !fin(dif) || !fin(qqq)) ok = false;
        }
        const float hsf = R0 / r_i;
        const float hsr = powr32(1.0f / hsf, pwr);
        hthick = fmaxf(hthick, dfl);
        if (i > 0 && !(fabsf(vs) > ACCUR)) hthick = 1.0e30f;   // a liquid layer below the top: exact kernel (entry_overflow_risk)
        rhomax = fmaxf(rhomax, rho * fmaxf(qqq, hsr));
        bmax = fmaxf(bmax, 1.06f * vs * fmaxf(dif, hsf));
        const size_t o = (size_t)i * B + b;
        const float v9[NF] = {vp, vs, rho, qs, dif, qqq, dfl, hsf, hsr};          // F_VP .. F_HSR
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            if (A.write_soa) mdl[f * fs + o] = v9[f];
            if (A.rows) A.rows[((size_t)b * NF + f) * Lmax + i] = v9[f];          // consecutive lanes: consecutive words
        }
    }
    // the stack's verdict and statistics over the lanes of its team
#pragma unroll
    for (int d = TL >> 1; d > 0; d >>= 1) {
        const int ok_o = __shfl_xor((int)ok, d), mono_o = __shfl_xor((int)mono, d);   // every lane shuffles
        ok = ok && (ok_o != 0);
        mono = mono && (mono_o != 0);
        hmax = fmaxf(hmax, __shfl_xor(hmax, d));
        hthick = fmaxf(hthick, __shfl_xor(hthick, d));
        rhomax = fmaxf(rhomax, __shfl_xor(rhomax, d));
        bmax = fmaxf(bmax, __shfl_xor(bmax, d));
    }
    if (valid && j == 0) {
        A.nl[b] = ok ? n : 0;          // 0 => BADMODEL: K1/K2 write zeros
        if (A.fsafe) A.fsafe[b] = (ok && mono) ? hmax : 1.0e30f;
        if (A.nsolved_init) A.nsolved_init[b] = ok ? A.P : 0;
        if (A.ovf) {
            A.ovf[b] = hthick;
            A.ovf[(size_t)B + b] = 2.0f * logf(fmaxf(rhomax, 1.0e-30f));
            A.ovf[2 * (size_t)B + b] = 4.0f * logf(fmaxf(2.0f * bmax * bmax, 1.0e-30f));
        }
        if (A.fb_count && b == 0) { A.fb_count[0] = 0; A.fb_count[1] = 0; A.fb_count[2] = 0; }
    }
}

// per-period, per-layer working values (calcul.f:112-131 then flat1 with n_flat layers)
struct LayerV { float a, b, rho, d; };

struct LayerRaw { float a_ref, b_ref, rho_ref, qs, dif, qqq, dfl, hsf, hsr; };

SD_HD __forceinline__ LayerRaw layer_load(const float *__restrict__ mdl, size_t fs, size_t o)
{
    LayerRaw r;
    r.a_ref = mdl[F_VP * fs + o];  r.b_ref = mdl[F_VS * fs + o];  r.rho_ref = mdl[F_RHO * fs + o];
    r.qs = mdl[F_QS * fs + o];     r.dif = mdl[F_DIF * fs + o];   r.qqq = mdl[F_QQQ * fs + o];
    r.dfl = mdl[F_DFL * fs + o];   r.hsf = mdl[F_HSF * fs + o];   r.hsr = mdl[F_HSR * fs + o];
    return r;
}

SD_HD __forceinline__ LayerV layer_derive(const LayerRaw &r, float lnT, bool is_halfspace)
{
#pragma clang fp contract(off)   // bit-identical at every call site (K2 integrates twice)
    const float qsq = r.qs * lnT / PI_REF;                                        // calcul.f:122
    const float qpq = qsq * 1.33333333f * (r.b_ref * r.b_ref) / (r.a_ref * r.a_ref); // calcul.f:123
    const float bb = r.b_ref * (1.0f + qsq);
    const float aa = r.a_ref * (1.0f + qpq);
    LayerV v;
    if (!is_halfspace) {
        v.a = aa * r.dif; v.b = bb * r.dif;
        v.rho = r.rho_ref * r.qqq;
        v.d = r.dfl;
    } else {
        v.a = aa * r.hsf; v.b = bb * r.hsf;
        v.rho = r.rho_ref * r.hsr;
        v.d = 0.0f;
    }
    return v;
}

SD_HD __forceinline__ LayerV layer_at(const float *__restrict__ mdl, size_t fs, size_t o,
                                           float lnT, bool is_halfspace)
{
    return layer_derive(layer_load(mdl, fs, o), lnT, is_halfspace);
}

}  // namespace sd
