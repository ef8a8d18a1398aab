// tests/hostcheck/eigencheck.hip -- test infrastructure only.
// The EIG instantiations of group_rayleigh / group_love (surfdisp_kernels.hip) compiled for the HOST, one row per unit
// (stride 1, planes Lmax words apart), so that the CPU tests can compare the layer-top eigenfunctions and the energy
// integrals with the reference's COMMON blocks (tests/golden/ref_eigen.npz).  Not linked into libsurfdisp_hip.so.
#include "../../pysurfinv_amd/csrc/surfdisp_kernels.hip"
#include <vector>

// out [B][P][4][Lmax]: the unit's stores as the lane leaves them (UNDIVIDED; entries the lane did not write stay as the
// caller filled them); unit [B][P][5] (double): divisor, deepest layer (-1: none), I0, I1, I2; u [B][P].
// Love: planes 0, 1 hold (ut, tq).  Units with c <= 0 or a bad stack are not run.
extern "C" int sd_eigencheck_group(int B, int Lmax, const int *nlay, const float *model, int P, const float *per, int kind,
                                   const float *c, const float *ratio, float *u, float *out, double *unit)
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
            const size_t o = (size_t)b * P + k;
            const sd::EOut eo{out + o * 4 * Lmax, 1, (size_t)Lmax};
            sd::EUnit eu{1.0f, -1, 0.0f, 0.0f, 0.0f};
            float ug = 0.0f, ks = 0.0f;
            int kh = -1;
            const sd::KOut ko{nullptr, 1, 0, 0, 0};
            if (nl[b] >= 2 && c[o] > 0.0f) {
                if (kind == 2) ug = sd::group_rayleigh<false, true>(mdl.data(), fs, B, b, nl[b], per[k], c[o], ratio[o], nullptr, ko, &ks, &kh, eo, &eu);
                else           ug = sd::group_love<false, true>(mdl.data(), fs, B, b, nl[b], per[k], c[o], ko, &ks, &kh, eo, &eu);
            }
            u[o] = ug;
            unit[o * 5 + 0] = eu.div; unit[o * 5 + 1] = eu.hs;
            unit[o * 5 + 2] = eu.i0; unit[o * 5 + 3] = eu.i1; unit[o * 5 + 4] = eu.i2;
        }
    return 0;
}

// Stand-alone run (for host sanitizer builds of this file as a program): a five-layer dry stack and a wet one, both wave
// types, at phase velocities inside the modes' range - not roots, but every store of the EIG instantiations runs.
int main()
{
    const int B = 2, L = 5, P = 2;
    const float model[B * 5 * L] = {
        5.0f, 6.0f, 6.5f, 7.8f, 8.1f,  2.9f, 3.5f, 3.8f, 4.4f, 4.6f,  2.5f, 2.7f, 2.9f, 3.3f, 3.4f,  2.0f, 10.0f, 15.0f, 20.0f, 0.0f,  0.005f, 0.003f, 0.002f, 0.002f, 0.002f,
        1.5f, 5.0f, 6.5f, 7.8f, 8.1f,  0.0f, 2.9f, 3.8f, 4.4f, 4.6f,  1.03f, 2.5f, 2.9f, 3.3f, 3.4f,  3.0f, 10.0f, 15.0f, 20.0f, 0.0f,  0.0f, 0.003f, 0.002f, 0.002f, 0.002f};
    const float per[P] = {10.0f, 30.0f};
    const float c[B * P] = {3.3f, 3.8f, 3.2f, 3.8f}, ratio[B * P] = {0.7f, 0.7f, 0.7f, 0.7f};
    std::vector<float> out((size_t)B * P * 4 * L, 0.0f), u(B * P);
    std::vector<double> unit(B * P * 5);
    for (int kind = 1; kind <= 2; ++kind) {
        sd_eigencheck_group(B, L, nullptr, model, P, per, kind, c, ratio, u.data(), out.data(), unit.data());
        for (int o = 0; o < B * P; ++o) printf("kind %d unit %d: U %.6f hs %d div %.6g I0 %.6g\n", kind, o, u[o], (int)unit[o * 5 + 1], unit[o * 5], unit[o * 5 + 2]);
    }
    return 0;
}
