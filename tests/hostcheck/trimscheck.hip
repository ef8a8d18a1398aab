// tests/hostcheck/trimscheck.hip -- test infrastructure only (tests/test_forward_trims_host.py): a stand-alone program.
// Compiles the group-velocity device math of surfdisp_kernels.hip for the HOST, like hostcheck.hip, and checks the two
// trims of the group kernel that change where a value comes from and not what it is:
//   trimscheck stash FILE   group_rayleigh with a host LStash buffer against group_rayleigh without one, unit by unit:
//                           U and the sixteen debug words (surface vectors, fit, energy integrals) byte for byte.
//                           FILE (text): B Lmax P / nlay[B] / model[B][5][Lmax] / per[P] / c[B][P] / ratio[B][P].
//   trimscheck drop N SEED  group_no_cut (the no-drop shortcut) against drop_group on N random (stack, c, T) of either
//                           wave type: wherever the shortcut fires the walk returns {n - 1, 0}.
// Prints one line per unit / one summary line; exit status 1 on any violation.  Not linked into libsurfdisp_hip.so.
struct SweepRec { int fits, fits_ref_split, mode1, mode2, mode1_kept, mode2_kept; };
static SweepRec *g_sweeps = nullptr;
#ifdef __HIP_DEVICE_COMPILE__
#define SD_SWEEP_PROBE(mode, own, kept) do { } while (0)
#else
#define SD_SWEEP_PROBE(mode, own, kept) \
    do { if (g_sweeps) { \
        if ((mode) == 0) { g_sweeps->fits++; if (!(own)) g_sweeps->fits_ref_split++; } \
        if ((mode) == 1) { g_sweeps->mode1++; if (kept) g_sweeps->mode1_kept++; } \
        if ((mode) == 2) { g_sweeps->mode2++; if (kept) g_sweeps->mode2_kept++; } } } while (0)
#endif
#include "../../pysurfinv_amd/csrc/surfdisp_kernels.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static int run_stash(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    int B, Lmax, P;
    if (fscanf(f, "%d %d %d", &B, &Lmax, &P) != 3) return 2;
    std::vector<int> nlay(B);
    std::vector<float> model((size_t)B * 5 * Lmax), per(P), c((size_t)B * P), ratio((size_t)B * P);
    for (auto &v : nlay) if (fscanf(f, "%d", &v) != 1) return 2;
    for (auto *a : {&model, &per, &c, &ratio})
        for (auto &v : *a) if (fscanf(f, "%g", &v) != 1) return 2;
    fclose(f);
    std::vector<float> mdl((size_t)10 * Lmax * B);
    std::vector<int> nl(B);
    sd::PrepArgs pa{B, Lmax, nlay.data(), model.data(), mdl.data(), nl.data()};
    pa.write_soa = 1;
    for (int b = 0; b < B; ++b) sd::prep_stack<2>(pa, b);
    const size_t fs = (size_t)Lmax * B;
    std::vector<float> buf((size_t)Lmax * SD_STASH_W);
    int bad = 0;
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < P; ++k) {
            const size_t i = (size_t)b * P + k;
            if (!(nl[b] >= 2 && c[i] > 0.0f)) continue;
            double d0[16], d1[16], d2[16];
            memset(d0, 0, sizeof d0); memset(d1, 0, sizeof d1); memset(d2, 0, sizeof d2);
            SweepRec r0{}, r1{};
            sd::KOut ko{nullptr, 1, 0, 0, 0};
            sd::EOut eo{nullptr, 1, 0};
            g_sweeps = &r0;
            const float u0 = sd::group_rayleigh<false, false, false>(mdl.data(), fs, B, b, nl[b], per[k], c[i], ratio[i], d0);
            // the stash starts out as garbage: a sweep may only read what this unit's own fit wrote
            memset(buf.data(), 0xAB, buf.size() * sizeof(float));
            sd::LStash st{buf.data(), 1};
            g_sweeps = &r1;
            const float u1 = sd::group_rayleigh<false, false, true>(mdl.data(), fs, B, b, nl[b], per[k], c[i], ratio[i], d1,
                                                                      ko, nullptr, nullptr, eo, nullptr, &st);
            g_sweeps = nullptr;
            // the stash instantiation handed no buffer: the recompute path again
            const float u2 = sd::group_rayleigh<false, false, true>(mdl.data(), fs, B, b, nl[b], per[k], c[i], ratio[i], d2);
            const bool same = memcmp(&u0, &u1, 4) == 0 && memcmp(d0, d1, sizeof d0) == 0 &&
                              memcmp(&u0, &u2, 4) == 0 && memcmp(d0, d2, sizeof d0) == 0;
            const bool sweeps = r0.fits == r1.fits && r0.fits_ref_split == r1.fits_ref_split && r0.mode1 == r1.mode1 &&
                                r0.mode2 == r1.mode2 && r0.mode1_kept == 0 && r0.mode2_kept == 0 &&
                                r1.mode1_kept == r1.mode1 && r1.mode2_kept == r1.mode2;
            uint32_t ub; memcpy(&ub, &u0, 4);
            printf("unit %d %d same %d sweeps %d u %08x hs %d nreg_hs %d fits %d ref_split_fits %d mode1 %d mode2 %d kept %d\n",
                   b, k, same ? 1 : 0, sweeps ? 1 : 0, ub, (int)d0[12], (int)d0[13], r1.fits, r1.fits_ref_split, r1.mode1,
                   r1.mode2, r1.mode1_kept + r1.mode2_kept);
            if (!same || !sweeps) ++bad;
        }
    return bad ? 1 : 0;
}

template <int KIND>
static void drop_one(std::mt19937 &rng, long *cnt)
{
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    const int Lmax = 24, B = 1;
    // layer counts up to 24: ndiv = 5 up to 20 layers, 4 beyond (Rayleigh)
    const int n = 2 + (int)(U(rng) * 22.999f);
    std::vector<float> model((size_t)5 * Lmax, 0.0f), mdl((size_t)10 * Lmax);
    const bool wet = U(rng) < 0.2f && n >= 3;
    const bool mono = U(rng) < 0.5f;
    float vs = 0.4f + 3.0f * U(rng);
    for (int i = 0; i < n; ++i) {
        vs = mono ? vs + 0.4f * U(rng) : 0.4f + 4.4f * U(rng);
        const float vp = vs * (1.6f + 0.8f * U(rng));
        model[0 * Lmax + i] = vp; model[1 * Lmax + i] = vs; model[2 * Lmax + i] = 0.541f + 0.3601f * vp;
        model[3 * Lmax + i] = (i == n - 1) ? 0.0f : 0.05f + 40.0f * U(rng) * U(rng);
        model[4 * Lmax + i] = (vs < 4.0f) ? 1.0f / 600.0f : 1.0f / 150.0f;
    }
    if (wet) { model[0] = 1.475f; model[1 * Lmax] = 0.0f; model[2 * Lmax] = 1.027f; model[4 * Lmax] = 1.0e-4f; }
    int nl = 0, nlay = n;
    sd::PrepArgs pa{B, Lmax, &nlay, model.data(), mdl.data(), &nl};
    pa.write_soa = 1;
    sd::prep_stack<KIND>(pa, 0);
    if (nl != n) { cnt[6]++; return; }
    const size_t fs = (size_t)Lmax * B;
    double tot = 0.0;
    for (int i = 0; i + 1 < n; ++i) tot += fabs((double)mdl[sd::F_DFL * fs + i]);
    // c anywhere between below the slowest and above the fastest layer; T from the ratio r = total thickness / (4 c T):
    // a third well below 1 (the shortcut fires), a third well above (it does not), a third within 2e-4 of 1
    const float c = 0.3f + 5.5f * U(rng);
    const float pick = U(rng);
    double r;
    if (pick < 1.0f / 3) r = 0.02 + 0.96 * U(rng);
    else if (pick < 2.0f / 3) r = 1.02 + 6.0 * U(rng);
    else r = 1.0 + 2.0e-4 * (2.0 * U(rng) - 1.0);
    const float T = (float)(tot / (4.0 * (double)c * r));
    const double rr = tot / (4.0 * (double)c * (double)T);            // the ratio as the floats have it
    // as group_rayleigh / group_love set the walk up
    const float lnT = logf(1.0f / T);
    int ndiv = 5;
    const int ivre = (KIND == 2 ? 99 : 999) / (n - 1);
    if (ndiv > ivre) ndiv = ivre;
    if (ndiv < 1) ndiv = 1;
    const float div = (float)ndiv;
    const sd::LayerV top = sd::layer_at(mdl.data(), fs, 0, lnT, false);
    const bool water = (ndiv > 1) ? (top.b <= 0.1e-10f) : false;
    const bool fire = sd::group_no_cut(mdl.data(), fs, B, 0, n, c, T);
    const sd::Drop w = sd::drop_group<KIND>(mdl.data(), fs, B, 0, n, lnT, c, T, ndiv, water, div);
    const bool nocut = (w.hs_layer == n - 1 && w.nreg_hs == 0);
    cnt[0]++;
    if (fire) cnt[1]++; else cnt[2]++;
    if (fire && !nocut) cnt[3]++;                                      // the violation
    if (fabs(rr - 1.0) <= 2.0e-4) { if (rr < 1.0) cnt[4]++; else cnt[5]++; }
    if (!nocut) cnt[7]++;
    if (!fire && nocut) cnt[8]++;                                      // (allowed: the walk found no cut either)
}

static int run_drop(long N, unsigned seed)
{
    std::mt19937 rng(seed);
    long cnt[9] = {0};
    for (long i = 0; i < N; ++i) { if (i & 1) drop_one<2>(rng, cnt); else drop_one<1>(rng, cnt); }
    printf("drop cases %ld fired %ld not_fired %ld violations %ld near_below %ld near_above %ld rejected %ld walk_cuts %ld walked_for_nothing %ld\n",
           cnt[0], cnt[1], cnt[2], cnt[3], cnt[4], cnt[5], cnt[6], cnt[7], cnt[8]);
    return cnt[3] ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "stash")) return run_stash(argv[2]);
    if (argc == 4 && !strcmp(argv[1], "drop")) return run_drop(atol(argv[2]), (unsigned)atol(argv[3]));
    fprintf(stderr, "usage: trimscheck stash FILE | trimscheck drop N SEED\n");
    return 2;
}
