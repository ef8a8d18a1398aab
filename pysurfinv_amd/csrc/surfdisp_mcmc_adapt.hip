// surfdisp_mcmc_adapt.hip -- adaptive Metropolis (Haario et al. 2001) pooled over the chains of a grid point: one update of the point's
// running mean and scatter from the chains' current states, a Robbins-Monro step of the log proposal scale from the accept flags of
// a window of track rows, and the scaled covariance surfdisp_mcmc_cov_factor_device factors into the proposal of
// surfdisp_mcmc_propose_cov_device (surfdisp_mcmc_adapt_device; include/surfdisp.h section (6c), "adaptive proposals").  A translation
// unit of its own: the kernels of surfdisp_mcmc.hip and surfdisp_mcmc_cov.hip keep their instruction streams
// (profiles/adaptive_proposal/isa_identity.txt).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "surfdisp_internal.h"

namespace sd {

// The Robbins-Monro step, every operation rounded on its own (no contraction: the numpy statement rounds each one too).
__device__ __forceinline__ double adapt_log_scale(double ls, double gain, double decay, double k, double a, double target,
                                                  double ls_min, double ls_max)
{
#pragma clang fp contract(off)
    const double g = gain * pow(k, -decay);
    const double inc = g * (a - target);
    return fmin(fmax(ls + inc, ls_min), ls_max);
}

// One workgroup = one wavefront = one point, lane n = scalar n (N <= 64), as surfdisp_mcmc_cov_factor_kernel: the scatter sits in LDS
// as T[k][n] (k <= n used: lane n owns column n, the lanes' accesses to one row are side by side), the chains of the point are fed
// one after the other in ascending order - W += 1; d = x - mean; mean += d / W; T[k][n] += d_k (x_n - mean_n) -, d goes from lane
// to lane through LDS (two buffers in turn: one barrier per chain).  No atomics, no private arrays, no scratch; the result does not
// depend on the launch shape (a point's sums are formed by one wavefront in one order).  The accept flags are counted as integers.
// LDS: N N + 128 doubles.
__global__ __launch_bounds__(64) void surfdisp_mcmc_adapt_kernel(McmcAdaptArgs A)
{
    extern __shared__ double lds[];                    // T [N][N], d [2][64]
    const int lane = threadIdx.x;
    const size_t pt = blockIdx.x;
    const int N = A.N, cpp = A.cpp;
    double *T = lds, *dl = lds + N * N;
    double *st = A.state + pt * (size_t)(SD_MCMC_ADAPT_HEAD + N + N * N);
    double *Sg = st + SD_MCMC_ADAPT_HEAD + N;
    const bool mine = lane < N;
    double W = st[0] * A.forget;
    for (int e = lane; e < N * N; e += 64) T[e] = Sg[e] * A.forget;
    double mean = mine ? st[SD_MCMC_ADAPT_HEAD + lane] : 0.0;
    __syncthreads();
    const double *x0 = A.p + pt * (size_t)cpp * N;
    double xn = mine ? x0[lane] : 0.0;
    for (int j = 0; j < cpp; ++j) {
        const double x = xn;
        if (mine && j + 1 < cpp) xn = x0[(size_t)(j + 1) * N + lane];   // (the next chain's row is on its way during this one's sums)
        double *db = dl + (j & 1) * 64;
        W += 1.0;
        const double d = x - mean;
        mean += d / W;
        const double e = x - mean;
        db[lane] = d;
        __syncthreads();
        if (mine)
            for (int k = 0; k <= lane; ++k) T[k * N + lane] += db[k] * e;
    }
    // the accept rate of the window: the flags of the point's chains, rows [row_lo, row_hi), counted as integers
    double ls = st[1], kk = st[2];
    const long nrow = (long)A.row_hi - A.row_lo;
    if (A.target_accept >= 0.0 && nrow > 0) {
        const long tot = (long)cpp * nrow;
        int cnt = 0;
        for (long i = lane; i < tot; i += 64) {
            const long j = i / nrow, r = A.row_lo + (i - j * nrow);
            cnt += A.track[((long)pt * cpp + j) * A.chain_stride + r * A.row_stride + 2] > 0.5 ? 1 : 0;
        }
        for (int m = 32; m > 0; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
        kk += 1.0;
        ls = adapt_log_scale(ls, A.gain, A.decay, kk, (double)cnt / (double)tot, A.target_accept, A.ls_min, A.ls_max);
    }
    const bool ready = W >= A.min_weight;
    __syncthreads();                                   // (every column of T is complete)
    for (int e = lane; e < N * N; e += 64) Sg[e] = T[e];
    if (mine) st[SD_MCMC_ADAPT_HEAD + lane] = mean;
    if (lane == 0) { st[0] = W; st[1] = ls; st[2] = kk; st[4] = ready ? 1.0 : 0.0; }
    if (!ready || A.cov_out == nullptr) return;
    // cov = exp(2 ls) (2.38^2 / N_live) (S / W + ridge diag(step^2)); a scalar whose diagonal is zero: zero row and column
    const double sn = mine ? A.step[lane] : 0.0;
    const double dn = mine ? T[lane * N + lane] / W + (A.ridge * sn) * sn : 0.0;
    const unsigned long long live = __ballot(mine && dn != 0.0);
    const int nlive = __popcll(live);
    const double c = nlive > 0 ? exp(2.0 * ls) * ((2.38 * 2.38) / (double)nlive) : 0.0;
    double *cov = A.cov_out + pt * (size_t)N * N;
    for (int e = lane; e < N * N; e += 64) {
        const int k = e / N, n = e - k * N;
        const int a = k < n ? k : n, b = k < n ? n : k;
        double v = 0.0;
        if (((live >> k) & 1) && ((live >> n) & 1)) {
            double base = T[a * N + b] / W;
            if (k == n) { const double s = A.step[n]; base += (A.ridge * s) * s; }
            v = c * base;
        }
        cov[e] = v;
    }
}

hipError_t launch_mcmc_adapt(hipStream_t s, const McmcAdaptArgs &a)
{
    const size_t bytes = ((size_t)a.N * a.N + 128) * sizeof(double);           // at most 33 KB (N = 64)
    hipLaunchKernelGGL(surfdisp_mcmc_adapt_kernel, dim3((unsigned)a.F), dim3(64), bytes, s, a);
    return hipGetLastError();
}

}  // namespace sd
