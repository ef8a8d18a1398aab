// tests/hostcheck/thickcheck.hip -- test infrastructure only.
// The unit function of the thickness kernel K2e (thick_unit / thick_interface of surfdisp_kernels.hip) compiled for the HOST,
// fed as the kernel feeds it: the KERN and the EIG instantiation of group_rayleigh / group_love leave one row per unit
// (stride 1, planes Lmax words apart), the suffix sum runs in fp64 from the deepest interface up.  Returns, beside dcdh and
// dcdz, the rows as the library's entries return them (K2b's fp32 products, K2d's fp32 quotients), so that the CPU tests can
// feed pysurfinv_amd.senskernel.thickness_kernels_reference with the same fp32 inputs.  Not linked into libsurfdisp_hip.so.
#include "../../pysurfinv_amd/csrc/surfdisp_kernels.hip"
#include <cmath>
#include <vector>

// per unit o = b * P + k:  u, i0 [B][P];  hs [B][P] (-1: a unit of zeros);  vt [B][P][4][Lmax] the layer-top values (Love:
// planes 0, 1 = ut, tq);  kb, ka, kr, dcdh, dcdz [B][P][Lmax].  Units with c <= 0 or a bad stack are rows of zeros.
extern "C" int sd_thickcheck_units(int B, int Lmax, const int *nlay, const float *model, int P, const float *per, int kind,
                                   const float *c, const float *ratio, float *u, float *i0, int *hs, float *vt,
                                   float *kb, float *ka, float *kr, float *dcdh, float *dcdz)
{
    std::vector<float> mdl((size_t)10 * Lmax * B);
    std::vector<int> nl(B);
    sd::PrepArgs pa{B, Lmax, nlay, model, mdl.data(), nl.data()};
    pa.write_soa = 1;
    for (int b = 0; b < B; ++b) {
        if (kind == 2) sd::prep_stack<2>(pa, b); else sd::prep_stack<1>(pa, b);
    }
    const size_t fs = (size_t)Lmax * B;
    std::vector<float> ev((size_t)4 * Lmax), kv((size_t)3 * Lmax);
    std::vector<double> dz((size_t)Lmax + 1);
    int bad_units = 0;
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < P; ++k) {
            const size_t o = (size_t)b * P + k, ro = o * Lmax;
            for (int i = 0; i < Lmax; ++i) { kb[ro + i] = ka[ro + i] = kr[ro + i] = dcdh[ro + i] = dcdz[ro + i] = 0.0f; }
            for (int i = 0; i < 4 * Lmax; ++i) vt[o * 4 * Lmax + i] = 0.0f;
            u[o] = 0.0f; i0[o] = 0.0f; hs[o] = -1;
            if (!(nl[b] >= 2 && c[o] > 0.0f)) continue;
            std::fill(ev.begin(), ev.end(), 0.0f); std::fill(kv.begin(), kv.end(), 0.0f);
            const sd::EOut eo{ev.data(), 1, (size_t)Lmax};
            const sd::EOut eo_none{nullptr, 1, 0};
            sd::EUnit eu{1.0f, -1, 0.0f, 0.0f, 0.0f}, eu_none = eu;
            const sd::KOut ko{kv.data(), 1, kind == 2 ? (ptrdiff_t)(Lmax * sizeof(float)) : 0, (ptrdiff_t)(2 * Lmax * sizeof(float)), 0};
            const sd::KOut ko_none{nullptr, 1, 0, 0, 0};
            float ug = 0.0f, ue = 0.0f, ks = 0.0f, ks2 = 0.0f;
            int kh = -1, kh2 = -1;
            if (kind == 2) {
                ug = sd::group_rayleigh<true, false>(mdl.data(), fs, B, b, nl[b], per[k], c[o], ratio[o], nullptr, ko, &ks, &kh, eo_none, &eu_none);
                ue = sd::group_rayleigh<false, true>(mdl.data(), fs, B, b, nl[b], per[k], c[o], ratio[o], nullptr, ko_none, &ks2, &kh2, eo, &eu);
            } else {
                ug = sd::group_love<true, false>(mdl.data(), fs, B, b, nl[b], per[k], c[o], ko, &ks, &kh, eo_none, &eu_none);
                ue = sd::group_love<false, true>(mdl.data(), fs, B, b, nl[b], per[k], c[o], ko_none, &ks2, &kh2, eo, &eu);
            }
            (void)ue;
            // what group_kernel_body stores per unit
            if (!(fabsf(ks) <= 3.0e38f)) ks = 0.0f;
            if (ks == 0.0f) kh = -1;
            if (!(fabsf(eu.i0) <= 3.0e38f) || !(fabsf(eu.i1) <= 3.0e38f) || !(fabsf(eu.i2) <= 3.0e38f)) eu = sd::EUnit{1.0f, -1, 0.0f, 0.0f, 0.0f};
            u[o] = ug; i0[o] = eu.i0;
            const sd::ThickUnit q = sd::thick_unit(mdl.data(), fs, B, b, nl[b], per[k], c[o], ug, eu.i0, eu.div, eu.hs, ks, kh,
                                                   ev.data(), 1, (size_t)Lmax, kv.data(), 1, (size_t)Lmax);
            hs[o] = q.hs;
            // the rows the entries return: K2b's products, K2d's quotients (with Love's low-amplitude exclusion)
            for (int i = 0; i <= kh; ++i) {
                kb[ro + i] = kv[i] * ks;
                if (kind == 2) ka[ro + i] = kv[Lmax + i] * ks;
                kr[ro + i] = kv[2 * Lmax + i] * ks;
            }
            const float lnT = logf(1.0f / per[k]);
            for (int i = 0; i <= eu.hs; ++i)
                for (int z = 0; z < (kind == 2 ? 4 : 2); ++z) {
                    float v = ev[(size_t)z * Lmax + i] / eu.div;
                    if (kind != 2 && fabsf(ev[i] / eu.div) < 1.0e-20f) {
                        const float vb = sd::layer_at(mdl.data(), fs, (size_t)i * B + b, lnT, i == nl[b] - 1).b;
                        const float vh = sd::layer_at(mdl.data(), fs, (size_t)eu.hs * B + b, lnT, eu.hs == nl[b] - 1).b;
                        if (vb >= vh) v = 0.0f;
                    }
                    vt[(o * 4 + z) * Lmax + i] = v;
                }
            if (q.hs < 1) continue;
            const float *h = model + ((size_t)b * 5 + 3) * Lmax;
            double z = 0.0;
            bool bad = false;
            for (int j = 1; j <= q.hs; ++j) {
                double kj;
                const float h_dn = (j < nl[b]) ? h[j] : 0.0f;
                dz[j] = (kind == 2) ? sd::thick_interface<2>(q, j, z, h[j - 1], h_dn, &kj) : sd::thick_interface<1>(q, j, z, h[j - 1], h_dn, &kj);
                if (!(std::fabs(dz[j]) <= 1.0e300)) bad = true;
                z = z + (double)h[j - 1];
            }
            double carry = 0.0;
            for (int j = q.hs; j >= 1; --j) {
                carry = carry + dz[j];
                dcdh[ro + j - 1] = (float)carry;
                dcdz[ro + j] = (float)dz[j];
            }
            if (bad) {
                ++bad_units;
                for (int i = 0; i < Lmax; ++i) dcdh[ro + i] = dcdz[ro + i] = std::nanf("");
            }
        }
    return bad_units;
}

// Stand-alone run (for host sanitizer builds of this file as a program): a five-layer dry stack and a wet one, both wave
// types, at phase velocities inside the modes' range - not roots, but every statement of the unit function runs.
int main()
{
    const int B = 2, L = 5, P = 2;
    const float model[B * 5 * L] = {
        5.0f, 6.0f, 6.5f, 7.8f, 8.1f,  2.9f, 3.5f, 3.8f, 4.4f, 4.6f,  2.5f, 2.7f, 2.9f, 3.3f, 3.4f,  2.0f, 10.0f, 15.0f, 20.0f, 0.0f,  0.005f, 0.003f, 0.002f, 0.002f, 0.002f,
        1.5f, 5.0f, 6.5f, 7.8f, 8.1f,  0.0f, 2.9f, 3.8f, 4.4f, 4.6f,  1.03f, 2.5f, 2.9f, 3.3f, 3.4f,  3.0f, 10.0f, 15.0f, 20.0f, 0.0f,  0.0f, 0.003f, 0.002f, 0.002f, 0.002f};
    const float per[P] = {10.0f, 30.0f};
    const float c[B * P] = {3.3f, 3.8f, 3.2f, 3.8f}, ratio[B * P] = {0.7f, 0.7f, 0.7f, 0.7f};
    std::vector<float> u(B * P), i0(B * P), vt((size_t)B * P * 4 * L), kb((size_t)B * P * L), ka(kb), kr(kb), dh(kb), dzr(kb);
    std::vector<int> hs(B * P);
    for (int kind = 1; kind <= 2; ++kind) {
        const int nb = sd_thickcheck_units(B, L, nullptr, model, P, per, kind, c, ratio, u.data(), i0.data(), hs.data(), vt.data(),
                                           kb.data(), ka.data(), kr.data(), dh.data(), dzr.data());
        for (int o = 0; o < B * P; ++o)
            printf("kind %d unit %d: U %.6f hs %d I0 %.6g dcdh %.6g %.6g %.6g %.6g (non-finite units %d)\n", kind, o, u[o], hs[o], i0[o],
                   dh[o * L], dh[o * L + 1], dh[o * L + 2], dh[o * L + 3], nb);
    }
    return 0;
}
