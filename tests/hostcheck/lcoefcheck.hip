// tests/hostcheck/lcoefcheck.hip -- test infrastructure only (tests/test_layer_coef_bits.py).
// Compiles layer_coef and sincos_cw of surfdisp_kernels.hip for the HOST and compares them, bit for bit, with the form they
// replace: r and 1/r signed by copysignf before the branch, the quadrant signs of sin and cos by selects.  v_rsq_f32 and
// v_exp_f32 become 1/sqrtf and exp2f on the host (rsq_hw, exp2_hw) in both forms alike, so what is compared is the sign
// and select handling around the unchanged fp32 arithmetic.  Not linked into libsurfdisp_hip.so.
#include "../../pysurfinv_amd/csrc/surfdisp_kernels.hip"
#include <cstdint>
#include <cstring>

namespace old_form {
static void sincos_cw(float x, float *sn, float *cs)
{
    const float TWO_OVER_PI = 6.36619747e-01f;
    const float P1 = 1.57079601e+00f, P2 = 3.13916473e-07f, P3 = 5.39030253e-15f;
    const float q = __builtin_rintf(x * TWO_OVER_PI);
    float r = fmaf(-q, P1, x);
    r = fmaf(-q, P2, r);
    r = fmaf(-q, P3, r);
    const int n = (int)q;
    const float r2 = r * r;
    float ps = fmaf(fmaf(fmaf(-1.9515295891e-4f, r2, 8.3321608736e-3f), r2, -1.6666654611e-1f), r2 * r, r);
    float pc = fmaf(fmaf(fmaf(2.443315711809948e-5f, r2, -1.388731625493765e-3f), r2, 4.166664568298827e-2f),
                    r2 * r2, fmaf(-0.5f, r2, 1.0f));
    const float s0 = (n & 1) ? pc : ps;
    const float c0 = (n & 1) ? ps : pc;
    *sn = (n & 2) ? -s0 : s0;
    *cs = ((n + 1) & 2) ? -c0 : c0;
}
static sd::LCoef layer_coef(const float arg, const float wd)
{
    const float xs = fmaxf(fabsf(arg), 1.0e-30f), y = sd::rsq_hw(xs);
    const float r = copysignf(xs * y, -arg), ir = copysignf(y, -arg);
    sd::LCoef o;
    o.r = r;
    o.x = wd * r;
    if (arg > 0.0f) {
        float sh, ch; sd::sinhcosh_sp(o.x, &sh, &ch);
        const float x2 = o.x * o.x;
        const float shs = fmaf(o.x * x2, fmaf(x2, 8.33333333e-3f, 1.66666667e-1f), o.x);
        if (fabsf(o.x) < 0.25f) sh = shs;
        o.rsin = -r * sh; o.sinr = sh * ir; o.cs = ch;
        o.ph = 0.0f;
    } else {
        float sn, cs; sincos_cw(o.x, &sn, &cs);
        o.rsin = r * sn; o.sinr = sn * ir; o.cs = cs;
        o.ph = o.x;
    }
    return o;
}
}  // namespace old_form

static inline uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static inline float fbits(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }
static inline bool same(float a, float b) { return (a != a && b != b) || bits(a) == bits(b); }   // NaN == NaN

// bit mask of the LCoef fields (r rsin sinr cs x ph) that differ between the two forms
static int lc_diff(float arg, float wd)
{
    const sd::LCoef a = old_form::layer_coef(arg, wd), b = sd::layer_coef(arg, wd);
    return (same(a.r, b.r) ? 0 : 1) | (same(a.rsin, b.rsin) ? 0 : 2) | (same(a.sinr, b.sinr) ? 0 : 4) |
           (same(a.cs, b.cs) ? 0 : 8) | (same(a.x, b.x) ? 0 : 16) | (same(a.ph, b.ph) ? 0 : 32);
}

static uint64_t splitmix(uint64_t &s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static inline double unif(uint64_t &s) { return (splitmix(s) >> 11) * (1.0 / 9007199254740992.0); }

extern "C" {
// the listed pairs: ndiff = number of pairs that differ; the first max_out of them go to idx / mask
int lc_pairs(long N, const float *arg, const float *wd, long max_out, long *idx, int *mask)
{
    long nd = 0;
    for (long i = 0; i < N; ++i) {
        const int m = lc_diff(arg[i], wd[i]);
        if (m) { if (nd < max_out) { idx[nd] = i; mask[nd] = m; } ++nd; }
    }
    return (int)(nd > 2147483647L ? 2147483647L : nd);
}
// N random pairs from seed: arg of either sign, |arg| log-uniform in [1e-12, 1e6] (1 in 64: a special value), k d log-uniform
// in [1e-6, 1e4]; the arg, wd of the first max_out differing pairs go to out_arg / out_wd
long lc_random(uint64_t seed, long N, long max_out, float *out_arg, float *out_wd)
{
    static const float special[] = {0.0f, -0.0f, 1.0e-30f, -1.0e-30f, 1.0e-40f, -1.0e-40f, 1.4e-45f, -1.4e-45f,
                                    INFINITY, -INFINITY, NAN, -NAN, 1.0f, -1.0f};
    const int ns = sizeof(special) / sizeof(special[0]);
    uint64_t s = seed;
    long nd = 0;
    for (long i = 0; i < N; ++i) {
        const uint64_t u = splitmix(s);
        float arg;
        if ((u & 63) == 0) arg = special[(u >> 8) % ns];
        else arg = (float)((u & 64 ? -1.0 : 1.0) * pow(10.0, -12.0 + 18.0 * unif(s)));
        const float wd = (float)pow(10.0, -6.0 + 10.0 * unif(s));
        if (lc_diff(arg, wd)) { if (nd < max_out) { out_arg[nd] = arg; out_wd[nd] = wd; } ++nd; }
    }
    return nd;
}
// every float x with bit pattern in [lo, hi) (x > 0) and its negative: the new sincos_cw against the old one (*nsame, first
// offender in *fsame) and odd in x to the bit, sincos_cw(-x) == (-sin x, cos x) (*nodd, first offender in *fodd)
void sincos_sweep(uint32_t lo, uint32_t hi, long *nsame, uint32_t *fsame, long *nodd, uint32_t *fodd)
{
    long ns = 0, no = 0;
    for (uint32_t u = lo; u < hi; ++u) {
        const float x = fbits(u);
        float sp, cp, sm, cm, op, ocp, om, ocm;
        sd::sincos_cw(x, &sp, &cp);
        sd::sincos_cw(-x, &sm, &cm);
        old_form::sincos_cw(x, &op, &ocp);
        old_form::sincos_cw(-x, &om, &ocm);
        if (!same(sp, op) || !same(cp, ocp) || !same(sm, om) || !same(cm, ocm)) { if (!ns) *fsame = u; ++ns; }
        if (!same(sm, -sp) || !same(cm, cp)) { if (!no) *fodd = u; ++no; }
    }
    *nsame = ns; *nodd = no;
}
}
