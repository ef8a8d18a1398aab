// tests/probe/secular_probe.hip -- TEST INFRASTRUCTURE ONLY.
// Runs the fp32 secular-function building blocks of surfdisp_kernels.hip on the GPU, one thread per case, so that
// tests/test_secular_functions.py can compare them with the float64 restatement in tests/secular64.py: the layer
// coefficients (layer_coef), one Rayleigh layer step (ray_step), the half-space closure (ray_close) and the whole
// secular functions (delta_rayleigh with both PIPE2 settings, delta_love) on a working stack in global memory (S = 1)
// formed with the rebuild's own expressions (wk_*).  It is not linked into libsurfdisp_hip.so and nothing in
// pysurfinv_amd/ loads it.  Every entry point takes and returns host arrays; the return value is a hipError_t.
#include "../../pysurfinv_amd/csrc/surfdisp_kernels.hip"

namespace {

constexpr int NW = 6;              // working-stack fields per layer (W_IR .. W_IB2); LS = NW, S = 1

__global__ void k_coef(int n, const float *arg, const float *wd, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const sd::LCoef o = sd::layer_coef(arg[i], wd[i]);
    float *q = out + (size_t)5 * i;
    q[0] = o.rsin; q[1] = o.sinr; q[2] = o.cs; q[3] = o.x; q[4] = o.ph;
}

// lyr[i] = (a, b, rho, d, rho_prev); flags[i] = start | first << 2
__global__ void k_step(int n, const float *st, const float *trial, const float *lyr, const int *flags, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *s = st + (size_t)5 * i, *y = lyr + (size_t)5 * i;
    const sd::RTrial t = sd::ray_trial(trial[2 * i], trial[2 * i + 1]);
    const sd::RLyr L{y[1], y[3], sd::wk_ia2(y[0]), sd::wk_ib2(y[1]), sd::wk_rat(y[4], y[2])};
    sd::RState r{s[0], s[1], s[2], s[3], s[4]};
    const int start = flags[i] & 3;
    float phi = 0.0f;
    if (flags[i] & 4) sd::ray_step<true>(r, t, L, start, phi); else sd::ray_step<false>(r, t, L, start, phi);
    float *q = out + (size_t)6 * i;
    q[0] = r.b1; q[1] = r.h2; q[2] = r.h3; q[3] = r.h4; q[4] = r.h5; q[5] = phi;
}

// lyr[i] = (a, b, rho, rho_prev) of the half space; start[i]; out = (value, mag)
__global__ void k_close(int n, const float *st, const float *trial, const float *lyr, const int *start, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *s = st + (size_t)5 * i, *y = lyr + (size_t)4 * i;
    const sd::RTrial t = sd::ray_trial(trial[2 * i], trial[2 * i + 1]);
    const sd::RLyr A{y[1], 0.0f, sd::wk_ia2(y[0]), sd::wk_ib2(y[1]), 0.0f};
    const sd::RState r{s[0], s[1], s[2], s[3], s[4]};
    float mag = 0.0f;
    out[2 * i] = sd::ray_close(r, t, A, y[2], y[3], start[i], &mag);
    out[2 * i + 1] = mag;
}

// stk[s] = a[L], b[L], rho[L], d[L]; the working stack of delta_rayleigh (kind 2) or delta_love (kind 1), as built in phase_body
__global__ void k_build(int nstk, int L, const float *stk, const int *mmax, int kind, float *wq)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nstk) return;
    const float *a = stk + (size_t)4 * L * s, *b = a + L, *rho = b + L, *d = rho + L;
    float *w = wq + (size_t)NW * L * s;
    for (int m = 0; m < mmax[s]; ++m) {
        float *q = w + NW * m;
        q[1] = b[m]; q[2] = rho[m]; q[3] = d[m];
        if (kind == 1) {
            q[0] = sd::wk_ilove(rho[m], b[m]); q[4] = 0.0f; q[5] = 0.0f;
        } else {
            q[0] = (m == 0) ? sd::wk_irho(rho[0]) : sd::wk_rat(rho[m - 1], rho[m]);
            q[4] = sd::wk_ia2(a[m]); q[5] = sd::wk_ib2(b[m]);
        }
    }
}

// mode 0: delta_rayleigh<PIPE2 = true>, 1: delta_rayleigh<PIPE2 = false>, 2: delta_love; out = (value, mag, phi)
__global__ void k_secular(int ntr, int L, const float *wq, const int *mmax, const int *tst, const float *c, const float *T,
                          int mode, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntr) return;
    const int s = tst[i];
    const float *w = wq + (size_t)NW * L * s;
    float phi = 0.0f, mag = 0.0f, v;
    if (mode == 2) {
        int kc = 0; bool kunc = false;
        v = sd::delta_love<false>(w, NW, 1, mmax[s], c[i], T[i], phi, kc, kunc, false, &mag);
    } else if (mode == 0) {
        v = sd::delta_rayleigh<true>(w, NW, 1, mmax[s], c[i], T[i], 1, phi, &mag);
    } else {
        v = sd::delta_rayleigh<false>(w, NW, 1, mmax[s], c[i], T[i], 1, phi, &mag);
    }
    out[3 * i] = v; out[3 * i + 1] = mag; out[3 * i + 2] = phi;
}

// device copies of host arrays, freed on scope exit
struct Dev {
    void *p[8] = {};
    int n = 0;
    hipError_t err = hipSuccess;
    template <class X> X *in(const X *h, size_t cnt)
    {
        void *q = nullptr;
        if (err == hipSuccess) err = hipMalloc(&q, cnt * sizeof(X) + 16);
        if (err == hipSuccess) err = hipMemcpy(q, h, cnt * sizeof(X), hipMemcpyHostToDevice);
        p[n++] = q;
        return (X *)q;
    }
    float *out(size_t cnt)
    {
        void *q = nullptr;
        if (err == hipSuccess) err = hipMalloc(&q, cnt * sizeof(float) + 16);
        if (err == hipSuccess) err = hipMemset(q, 0, cnt * sizeof(float));
        p[n++] = q;
        return (float *)q;
    }
    hipError_t fetch(float *h, const float *d, size_t cnt)
    {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
        if (err == hipSuccess) err = hipMemcpy(h, d, cnt * sizeof(float), hipMemcpyDeviceToHost);
        return err;
    }
    ~Dev() { for (int i = 0; i < n; ++i) if (p[i]) (void)hipFree(p[i]); }
};
inline int nblk(int n) { return (n + 255) / 256; }

}  // namespace

extern "C" int sp_coef(int n, const float *arg, const float *wd, float *out)
{
    if (n <= 0) return 0;
    Dev D;
    const float *da = D.in(arg, n), *dw = D.in(wd, n);
    float *o = D.out((size_t)5 * n);
    if (D.err == hipSuccess) hipLaunchKernelGGL(k_coef, dim3(nblk(n)), dim3(256), 0, 0, n, da, dw, o);
    return (int)D.fetch(out, o, (size_t)5 * n);
}

extern "C" int sp_step(int n, const float *st, const float *trial, const float *lyr, const int *flags, float *out)
{
    if (n <= 0) return 0;
    Dev D;
    const float *ds = D.in(st, (size_t)5 * n), *dt = D.in(trial, (size_t)2 * n), *dl = D.in(lyr, (size_t)5 * n);
    const int *df = D.in(flags, n);
    float *o = D.out((size_t)6 * n);
    if (D.err == hipSuccess) hipLaunchKernelGGL(k_step, dim3(nblk(n)), dim3(256), 0, 0, n, ds, dt, dl, df, o);
    return (int)D.fetch(out, o, (size_t)6 * n);
}

extern "C" int sp_close(int n, const float *st, const float *trial, const float *lyr, const int *start, float *out)
{
    if (n <= 0) return 0;
    Dev D;
    const float *ds = D.in(st, (size_t)5 * n), *dt = D.in(trial, (size_t)2 * n), *dl = D.in(lyr, (size_t)4 * n);
    const int *dst = D.in(start, n);
    float *o = D.out((size_t)2 * n);
    if (D.err == hipSuccess) hipLaunchKernelGGL(k_close, dim3(nblk(n)), dim3(256), 0, 0, n, ds, dt, dl, dst, o);
    return (int)D.fetch(out, o, (size_t)2 * n);
}

// stk: nstk x [4][L] (a, b, rho, d); mmax[s] in 2..L; tst[i] in 0..nstk-1 (checked here: the kernels index with them)
extern "C" int sp_secular(int nstk, int L, const float *stk, const int *mmax, int ntr, const int *tst, const float *c,
                          const float *T, int kind, int mode, float *out)
{
    if (nstk <= 0 || ntr <= 0 || L < 2) return 0;
    for (int s = 0; s < nstk; ++s) if (mmax[s] < 2 || mmax[s] > L) return (int)hipErrorInvalidValue;
    for (int i = 0; i < ntr; ++i) if (tst[i] < 0 || tst[i] >= nstk) return (int)hipErrorInvalidValue;
    if (!((kind == 2 && (mode == 0 || mode == 1)) || (kind == 1 && mode == 2))) return (int)hipErrorInvalidValue;
    Dev D;
    const float *dstk = D.in(stk, (size_t)4 * L * nstk), *dc = D.in(c, ntr), *dT = D.in(T, ntr);
    const int *dm = D.in(mmax, nstk), *dts = D.in(tst, ntr);
    float *wq = D.out((size_t)NW * L * nstk);
    float *o = D.out((size_t)3 * ntr);
    if (D.err == hipSuccess) hipLaunchKernelGGL(k_build, dim3(nblk(nstk)), dim3(256), 0, 0, nstk, L, dstk, dm, kind, wq);
    if (D.err == hipSuccess) hipLaunchKernelGGL(k_secular, dim3(nblk(ntr)), dim3(256), 0, 0, ntr, L, wq, dm, dts, dc, dT, mode, o);
    return (int)D.fetch(out, o, (size_t)3 * ntr);
}
