// tests/hostcheck/powcheck.hip -- test infrastructure only (tests/test_group_powers.py).
// Compiles the closed-form RK4 powers of surfdisp_kernels.hip (make_base / pow_sublayers / pow_expand) for the HOST and
// returns, for each layer's coefficients and sublayer count nreg, P^(4 nreg) three ways, each as the blocks p11 p12 p21 p22
// (16 doubles, block order x = (ur, tz), w = (uz, tr)):
//   closed:  the closed form the group kernel's fit uses;
//   stepped: P^4 = prop_sq(prop_sq(make_prop)) applied nreg times with prop_apply (the fit before the closed form);
//   ref:     long double: P = I + k1 A + k2 A^2 + k3 A^3 + k4 A^4 from the same k1..k4 and A, then 4 nreg - 1 products.
// Not linked into libsurfdisp_hip.so.
#include "../../pysurfinv_amd/csrc/surfdisp_kernels.hip"

static void put_blocks(const sd::RProp &P, double *o)
{
    const sd::M2x2 *m[4] = {&P.p11, &P.p12, &P.p21, &P.p22};
    for (int i = 0; i < 4; ++i) { o[4 * i] = m[i]->a; o[4 * i + 1] = m[i]->b; o[4 * i + 2] = m[i]->c; o[4 * i + 3] = m[i]->d; }
}

typedef long double LD;
static void mat4(const LD *x, const LD *y, LD *r)
{
    LD t[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            LD s = 0;
            for (int k = 0; k < 4; ++k) s += x[4 * i + k] * y[4 * k + j];
            t[4 * i + j] = s;
        }
    for (int i = 0; i < 16; ++i) r[i] = t[i];
}

// q9: a12 a13 a21 a24 a31 a34 a42 a43 ddz per layer (RCoef order)
extern "C" int sd_powcheck(int N, const float *q9, const int *nreg, double *closed, double *stepped, double *ref)
{
    for (int l = 0; l < N; ++l) {
        const float *f = q9 + 9 * (size_t)l;
        const sd::RCoef q{f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8]};
        const int nr = nreg[l];
        const sd::RBase L = sd::make_base(q);
        put_blocks(sd::pow_expand(L, sd::pow_sublayers(L, nr)), closed + 16 * (size_t)l);

        const sd::RProp P4 = sd::prop_sq(sd::prop_sq(sd::make_prop(q)));
        sd::RProp S;
        sd::M2x2 *blk[4] = {&S.p11, &S.p12, &S.p21, &S.p22};
        const int vi[4] = {0, 2, 1, 3};                       // block order (ur, tz, uz, tr) -> prop_apply's (ur, uz, tz, tr)
        for (int j = 0; j < 4; ++j) {
            double v[4] = {0, 0, 0, 0};
            v[vi[j]] = 1.0;
            for (int s = 0; s < nr; ++s) sd::prop_apply(P4, v);
            for (int i = 0; i < 4; ++i) {                     // entry (i, j) of the 4x4 in block order
                double *e = &(blk[2 * (i / 2) + j / 2]->a);
                e[2 * (i % 2) + (j % 2)] = v[vi[i]];
            }
        }
        put_blocks(S, stepped + 16 * (size_t)l);

        // the same k1..k4 (from the fp32 weights, as make_prop forms them) and A, in long double
        const LD wh = (double)(0.5f * q.ddz), w1 = (double)(1.0f * q.ddz);
        const LD t6 = (double)((1.0f / 6.0f) * q.ddz), t3 = (double)((1.0f / 3.0f) * q.ddz);
        const LD k[5] = {1, (t6 + t3) + (t3 + t6), (t3 * wh + t3 * wh) + t6 * w1, t3 * wh * wh + t6 * w1 * wh, t6 * w1 * wh * wh};
        LD A[16] = {0};
        A[0 * 4 + 2] = q.a31; A[0 * 4 + 3] = q.a34; A[1 * 4 + 2] = q.a21; A[1 * 4 + 3] = q.a24;   // x' = M1 w
        A[2 * 4 + 0] = q.a13; A[2 * 4 + 1] = q.a12; A[3 * 4 + 0] = q.a43; A[3 * 4 + 1] = q.a42;   // w' = M2 x
        LD Ak[16], P[16];
        for (int i = 0; i < 16; ++i) { Ak[i] = (i % 5 == 0) ? 1 : 0; P[i] = Ak[i]; }
        for (int p = 1; p <= 4; ++p) {
            mat4(Ak, A, Ak);
            for (int i = 0; i < 16; ++i) P[i] += k[p] * Ak[i];
        }
        LD R[16];
        for (int i = 0; i < 16; ++i) R[i] = P[i];
        for (int m = 1; m < 4 * nr; ++m) mat4(R, P, R);
        double *o = ref + 16 * (size_t)l;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) o[4 * (2 * (i / 2) + j / 2) + 2 * (i % 2) + (j % 2)] = (double)R[4 * i + j];
    }
    return 0;
}
