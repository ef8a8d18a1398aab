// tests/hostcheck/splitcheck.hip -- test infrastructure only (tests/test_group_split.py).
// Compiles the group-velocity device math of surfdisp_kernels.hip for the HOST, like hostcheck.hip, and records for every
// unit on the fast path the sublayer counts of its energy-integral sweep: for each layer jl the reference's count nreg
// and the count n' the sweep stepped (fast_sublayers).  Built twice by the test: with the default SD_GROUP_LAMH and with
// -DSD_GROUP_LAMH=0 (the reference's split everywhere).  Not linked into libsurfdisp_hip.so.
static int *g_rec = nullptr;    // this unit's record: [Lmax][2] (nreg, n'), -1 where the sweep did not step a layer
#ifdef __HIP_DEVICE_COMPILE__
#define SD_SPLIT_PROBE(nreg, nstep) do { } while (0)
#else
#define SD_SPLIT_PROBE(nreg, nstep) \
    do { if (g_rec) { g_rec[2 * jl] = (nreg); g_rec[2 * jl + 1] = (nstep); } } while (0)
#endif
#include "../../pysurfinv_amd/csrc/surfdisp_kernels.hip"
#include <vector>

// model [B][5][Lmax], nlay [B] (nullptr: every stack Lmax layers); c, ratio, u [B][P]; hs [B][P] (the layer that holds the half space);
// rec [B][P][Lmax][2]
extern "C" int sd_splitcheck_group(int B, int Lmax, const int *nlay, const float *model, int P, const float *per, const float *c,
                                   const float *ratio, float *u, int *hs, int *rec, double *cancel)
{
    std::vector<float> mdl((size_t)10 * Lmax * B);
    std::vector<int> nl(B);
    sd::PrepArgs pa{B, Lmax, nlay, model, mdl.data(), nl.data()};
    pa.write_soa = 1;
    for (int b = 0; b < B; ++b) sd::prep_stack<2>(pa, b);
    const size_t fs = (size_t)Lmax * B;
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < P; ++k) {
            const size_t i = (size_t)b * P + k;
            int *r = rec + 2 * (size_t)Lmax * i;
            for (int j = 0; j < 2 * Lmax; ++j) r[j] = -1;
            const float cc = c[i];
            double dbg[16] = {0};
            float ug = 0.0f;
            hs[i] = -1;
            if (cancel) cancel[i] = 0.0;
            if (nl[b] >= 2 && cc > 0.0f) {
                g_rec = r;
                ug = sd::group_rayleigh(mdl.data(), fs, B, b, nl[b], per[k], cc, ratio[i], dbg);
                g_rec = nullptr;
                hs[i] = (int)dbg[12];
                if (cancel)                                   // the fit's growth over the normalisation (group_rayleigh)
                    cancel[i] = fmax(fmax(fabs(dbg[0]), fabs(dbg[1])), fmax(fabs(dbg[4]), fabs(dbg[5]))) / fabs(dbg[9]);
            }
            u[i] = ug;
        }
    return 0;
}
