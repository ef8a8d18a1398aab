// tests/hostcheck/hostcheck.hip -- DEBUG HARNESS, test infrastructure only.
// Compiles the group-velocity device math of surfdisp_kernels.hip for the HOST so that it can be
// stepped through / compared with the oracle in the CPU-only development container.  It is not
// linked into libsurfdisp_hip.so and nothing in pysurfinv_amd/ loads it.
#include "../../pysurfinv_amd/csrc/surfdisp_kernels.hip"
#include <vector>
#include <cstdlib>

// prep_stack's nine per-layer fields (vp, vs, rho, 1/Qs, dif, qqq, dfl, hsf, hsr), one row per stack and field:
// rows [B][9][Lmax], zero-filled first (prep_stack writes layers < nlay of a valid stack); nl [B] as prep_stack leaves it.
extern "C" int sd_hostcheck_prep_rows(int B, int Lmax, const int *nlay, const float *model, int kind, float *rows, int *nl)
{
    for (size_t i = 0; i < (size_t)B * 9 * Lmax; ++i) rows[i] = 0.0f;
    sd::PrepArgs pa{B, Lmax, nlay, model, nullptr, nl};
    pa.rows = rows;
    pa.write_soa = 0;
    for (int b = 0; b < B; ++b) {
        if (kind == 2) sd::prep_stack<2>(pa, b); else sd::prep_stack<1>(pa, b);
    }
    return 0;
}

// prep_stack's per-stack verdict and statistics: nl [B], fsafe [B], ovf [3][B]
extern "C" int sd_hostcheck_prep_stats(int B, int Lmax, const int *nlay, const float *model, int kind, int *nl, float *fsafe, float *ovf)
{
    std::vector<float> rows((size_t)B * 9 * Lmax);
    sd::PrepArgs pa{B, Lmax, nlay, model, nullptr, nl};
    pa.rows = rows.data();
    pa.write_soa = 0;
    pa.fsafe = fsafe;
    pa.ovf = ovf;
    for (int b = 0; b < B; ++b) {
        if (kind == 2) sd::prep_stack<2>(pa, b); else sd::prep_stack<1>(pa, b);
    }
    return 0;
}

extern "C" int sd_hostcheck_group(int B, int Lmax, const int *nlay, const float *model, int P,
                                  const float *per, int kind, const float *c, const float *ratio,
                                  float *u, double *dbg)
{
    std::vector<float> mdl((size_t)10 * Lmax * B);
    std::vector<int> nl(B);
    sd::PrepArgs pa{B, Lmax, nlay, model, mdl.data(), nl.data()};
    pa.write_soa = 1;
    for (int b = 0; b < B; ++b) {
        if (kind == 2) sd::prep_stack<2>(pa, b); else sd::prep_stack<1>(pa, b);
    }
    const size_t fs = (size_t)Lmax * B;
    if (const char *e = getenv("SD_PERT_FIELD")) {       // sensitivity probe: scale one SoA field
        const int f = atoi(e); const float eps = (float)atof(getenv("SD_PERT_EPS"));
        for (size_t i = 0; i < fs; ++i) mdl[f * fs + i] *= (1.0f + eps);
    }
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < P; ++k) {
            const float cc = c[(size_t)b * P + k];
            float ug = 0.0f;
            if (nl[b] >= 2 && cc > 0.0f) {
                if (kind == 2) ug = sd::group_rayleigh(mdl.data(), fs, B, b, nl[b], per[k], cc, ratio[(size_t)b * P + k], dbg ? dbg + 16 * ((size_t)b * P + k) : nullptr);
                else           ug = sd::group_love(mdl.data(), fs, B, b, nl[b], per[k], cc);
            }
            u[(size_t)b * P + k] = ug;
        }
    return 0;
}

// The group-velocity kernel's KERN instantiation on the direct route (one row per unit, scaled by the lane itself as
// surfdisp_group_kernel does): u [B][P] and the partials kb, ka, kr [B][P][Lmax] at the given roots and ellipticities;
// rawc != 0: SURFDISP_KERN_REFCOORD (unit chain factors).  Love: ka is zeros.
// group_rayleigh / group_love, kern_coef and chain_of are the kernel's own; the KOut set-up and the lines after the call
// (the kscale clamp, top = khs, scaling and zero fill) MIRROR surfdisp_group_kernel's direct route ("direct route: the lane
// finishes its own rows") and are not the code under test - tests/test_kernel_rows_gpu.py runs that on the device.
extern "C" int sd_hostcheck_kernels(int B, int Lmax, const int *nlay, const float *model, int P, const float *per, int kind,
                                    int rawc, const float *c, const float *ratio, float *u, float *kb, float *ka, float *kr)
{
    std::vector<float> mdl((size_t)10 * Lmax * B);
    std::vector<int> nl(B);
    sd::PrepArgs pa{B, Lmax, nlay, model, mdl.data(), nl.data()};
    pa.write_soa = 1;
    for (int b = 0; b < B; ++b) {
        if (kind == 2) sd::prep_stack<2>(pa, b); else sd::prep_stack<1>(pa, b);
    }
    const size_t fs = (size_t)Lmax * B;
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < P; ++k) {
            const size_t ro = ((size_t)b * P + k) * Lmax;
            sd::KOut ko{kb + ro, 1, (kind == 2) ? (ptrdiff_t)((char *)ka - (char *)kb) : 0, (ptrdiff_t)((char *)kr - (char *)kb), rawc};
            const float cc = c[(size_t)b * P + k];
            float ug = 0.0f, kscale = 0.0f;
            int khs = -1;
            if (nl[b] >= 2 && cc > 0.0f) {
                if (kind == 2) ug = sd::group_rayleigh<true>(mdl.data(), fs, B, b, nl[b], per[k], cc, ratio[(size_t)b * P + k], nullptr, ko, &kscale, &khs);
                else           ug = sd::group_love<true>(mdl.data(), fs, B, b, nl[b], per[k], cc, ko, &kscale, &khs);
            }
            if (!(fabsf(kscale) <= 3.0e38f)) kscale = 0.0f;
            const int top = (kscale != 0.0f) ? khs : -1;
            for (int i = 0; i < Lmax; ++i) {
                kb[ro + i] = (i <= top) ? kb[ro + i] * kscale : 0.0f;
                ka[ro + i] = (kind == 2 && i <= top) ? ka[ro + i] * kscale : 0.0f;
                kr[ro + i] = (i <= top) ? kr[ro + i] * kscale : 0.0f;
            }
            u[(size_t)b * P + k] = ug;
        }
    return 0;
}
