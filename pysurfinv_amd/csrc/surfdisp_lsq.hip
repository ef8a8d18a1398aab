// surfdisp_lsq.hip -- one damped, smoothed least-squares (Gauss-Newton / Levenberg-Marquardt) step of the free layers' Vs of
// every stack of a batch, on the device (include/surfdisp.h section (6d); the host statement of the same step is
// pysurfinv_amd.linearized.lsq_step_reference).  The consumer of the analytic sensitivity kernels (sections (5b)-(5d)): their
// [B][P][Lmax] fp32 partial arrays and the solves' predictions go in as they are, the step comes out, nothing visits the host.
//
// One workgroup of 256 lanes per stack.  With n free layers and the data rows r of the joint column table
// (surfdisp_mcmc_accept_joint5_device), the AUGMENTED matrix [G | res]^T W [G | res] (n + 1 columns: the effective Jacobian
// row G[r,i] = K_b + p_i K_a + q_i K_rho and the residual) is accumulated in fp64 into the packed lower triangle M of LDS,
// row i at i (i + 1) / 2: rows 0..n-1 are G^T W G, row n holds G^T W res and, last, the data misfit res^T W res.  The rows are
// staged 16 at a time in LDS ([16][n + 1] doubles), where a row with a non-finite entry is found and dropped before it is
// summed.  Then alpha D^T Q D + lambda I goes onto the band, -alpha D^T Q D x0 onto row n, and a right-looking Cholesky
// factorisation runs over the columns 0..n-1 of all n + 1 rows: row n comes out as y = L^-1 g (the forward substitution is
// the factorisation's own trailing update), and one back substitution L^T delta = y remains.
// LDS traffic: the trailing update of column k reads the scaled column from a contiguous copy (cv) - lanes 0..15 of a group
// read 16 consecutive doubles, the four groups of a wavefront one broadcast value each - and updates 16 consecutive doubles
// of a packed row: no strided column sweep, so no bank conflicts beyond the chance overlap of the four rows' offsets.  The
// column scaling itself (n - k strided elements, once per column) is the only strided access.
// Everything indexed by layer or row lives in LDS: no private arrays, no scratch (tests/test_isa_guard.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "surfdisp_internal.h"

namespace sd {

__device__ __forceinline__ int lsq_tri(int i, int j) { return i * (i + 1) / 2 + j; }      // j <= i
__device__ __forceinline__ bool lsq_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

size_t lsq_lds_bytes(int nmax)
{
    return ((size_t)(nmax + 1) * (nmax + 2) / 2 + (size_t)SD_LSQ_TILE_ROWS * (nmax + 1)) * sizeof(double);
}

__global__ __launch_bounds__(256) void surfdisp_lsq_step_kernel(LsqArgs A)
{
    constexpr int R = SD_LSQ_TILE_ROWS, NF = SD_LSQ_MAX_FREE + 1;
    extern __shared__ double lsq_smem[];
    __shared__ double x0[NF], ps[NF], qs[NF], qw[NF], cv[NF], dg[NF], dl[NF];
    __shared__ int fidx[NF], pos[SURFDISP_NLAY_MAX];
    __shared__ const float *rkb[R], *rka[R], *rkr[R];
    __shared__ double rwr[R], rsg[R], rt[R];
    __shared__ int rok[R], rbad[R];
    __shared__ int sh_n, sh_over, sh_flag;

    const int s = blockIdx.x, tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int Lmax = A.Lmax;
    int nl = A.nlay ? A.nlay[s] : Lmax;
    nl = nl < 0 ? 0 : (nl > Lmax ? Lmax : nl);
    const size_t ob = A.obs_per_stack ? (size_t)s * A.N : 0;

    // ---- the free layers of this stack, in order: fidx[j] = layer of unknown j, pos[layer] = j or -1
    for (int i = tid; i < Lmax; i += 256) pos[i] = -1;
    __syncthreads();
    if (tid < 64) {
        const unsigned char *fm = A.free_mask ? A.free_mask + (A.free_per_stack ? (size_t)s * Lmax : 0) : nullptr;
        int cnt = 0;
        for (int base = 0; base < nl; base += 64) {
            const int i = base + tid;
            const bool f = i < nl && (!fm || fm[i] != 0);
            const unsigned long long m = __ballot(f);
            const int k = cnt + __popcll(m & ((1ull << tid) - 1ull));
            if (f && k < A.nmax) { fidx[k] = i; pos[i] = k; }
            cnt += __popcll(m);
        }
        if (tid == 0) { sh_n = cnt < A.nmax ? cnt : A.nmax; sh_over = cnt > A.nmax ? 1 : 0; sh_flag = 0; }
    }
    __syncthreads();
    const int n = sh_n;
    double *delta = A.delta + (size_t)s * Lmax;
    if (sh_over) {                                   // more free layers than the caller sized the launch for: nothing is solved
        for (int i = tid; i < Lmax; i += 256) delta[i] = 0.0;
        if (tid == 0) {
            A.stats[3 * (size_t)s] = 0.0; A.stats[3 * (size_t)s + 1] = 0.0; A.stats[3 * (size_t)s + 2] = 0.0;
            A.info[3 * (size_t)s] = 0; A.info[3 * (size_t)s + 1] = A.N; A.info[3 * (size_t)s + 2] = 3;
        }
        return;
    }
    const int n1 = n + 1;
    double *M = lsq_smem;                            // packed lower triangle of the (n + 1) x (n + 1) augmented matrix
    double *Gt = lsq_smem + (size_t)(A.nmax + 1) * (A.nmax + 2) / 2;   // [R][n1]: staged rows, column n = residual
    const int tot = n1 * (n1 + 1) / 2;

    {
        const float *vs = A.model + ((size_t)s * 5 + 1) * Lmax;
        const double *vps = A.vp_slope ? A.vp_slope + (A.slope_per_stack ? (size_t)s * Lmax : 0) : nullptr;
        const double *rhs = A.rho_slope ? A.rho_slope + (A.slope_per_stack ? (size_t)s * Lmax : 0) : nullptr;
        const double *Q = A.Q ? A.Q + (A.q_per_stack ? (size_t)s * (Lmax - 1) : 0) : nullptr;
        for (int j = tid; j < n; j += 256) {
            const int i = fidx[j];
            x0[j] = (double)vs[i];
            ps[j] = vps ? vps[i] : 0.0;
            qs[j] = rhs ? rhs[i] : 0.0;
            if (j + 1 < n) {                         // the weakest interface between two consecutive free layers
                double m = Q ? Q[i] : 1.0;
                for (int k = i + 1; k < fidx[j + 1]; ++k) m = (Q && Q[k] < m) ? Q[k] : m;
                qw[j] = m;
            }
        }
        for (int t = tid; t < tot; t += 256) M[t] = 0.0;
    }
    __syncthreads();

    // stage the rows r0 .. r0 + R - 1: validity, weight, residual, effective Jacobian row
    auto stage = [&](int r0) {
        if (tid < R) {
            const int r = r0 + tid;
            int ok = 0;
            double wr = 0.0, sg = 1.0, res = 0.0;
            const float *kb = nullptr, *ka = nullptr, *kr = nullptr;
            if (r < A.N) {
                const int src = A.cols[2 * r], idx = A.cols[2 * r + 1];
                const int sa = src == 5 ? 4 : src;                         // sources 4 and 5 read the same solve's chi
                const float *pp = nullptr;
                long pst = 0;
#pragma unroll
                for (int k = 0; k < 5; ++k)
                    if (k == sa) { pp = A.pred[k]; pst = A.pstride[k]; kb = A.part[3 * k]; ka = A.part[3 * k + 1]; kr = A.part[3 * k + 2]; }
                const int P = (sa >= 0 && sa <= 4) ? (sa >= 2 && sa <= 3 ? A.nper[1] : A.nper[0]) : 0;
                const double o = A.obs[ob + r], sgm = A.uncer[ob + r];
                const bool in = A.mask[ob + r] != 0 && lsq_finite(o) && lsq_finite(sgm) && sgm > 0.0;
                if (pp && in && idx >= 0 && idx < P) {
                    double v = (double)pp[(size_t)s * pst + idx];
                    bool solved;
                    if (sa == 4) {                                          // chi: finite, at a period whose root was found
                        solved = lsq_finite(v) && (double)A.pred[0][(size_t)s * A.pstride[0] + idx] >= 0.01;
                        if (src == 5 && v < 0.0) { sg = -1.0; v = -v; }     // |chi|: the row takes the sign of chi
                    } else
                        solved = v >= 0.01;
                    if (solved) {
                        ok = 1;
                        wr = A.weights[r] / (sgm * sgm);
                        res = o - v;
                        const size_t off = ((size_t)s * P + idx) * Lmax;
                        kb = kb ? kb + off : nullptr; ka = ka ? ka + off : nullptr; kr = kr ? kr + off : nullptr;
                    }
                }
            }
            rok[tid] = ok; rbad[tid] = 0; rwr[tid] = wr; rsg[tid] = sg;
            rkb[tid] = kb; rka[tid] = ka; rkr[tid] = kr;
            Gt[tid * n1 + n] = res;
        }
        __syncthreads();
        for (int t = tid; t < R * n; t += 256) {
            const int rr = t / n, j = t - rr * n;
            if (rok[rr]) {
                const int i = fidx[j];
                const float *kb = rkb[rr], *ka = rka[rr], *kr = rkr[rr];
                double g = kb ? (double)kb[i] : 0.0;
                if (ka && ps[j] != 0.0) g += ps[j] * (double)ka[i];
                if (kr && qs[j] != 0.0) g += qs[j] * (double)kr[i];
                g *= rsg[rr];
                if (!lsq_finite(g)) rbad[rr] = 1;                           // a NaN row of a failed unit: dropped
                Gt[rr * n1 + j] = g;
            }
        }
        __syncthreads();
        if (tid < R) {
            const int fin = rok[tid] && !rbad[tid];
            rok[tid] = fin;
            if (!fin) rwr[tid] = 0.0;
        }
        __syncthreads();
    };

    // ---- [G | res]^T W [G | res] into M
    int used = 0;                                                          // (thread 0's copy counts)
    for (int r0 = 0; r0 < A.N; r0 += R) {
        stage(r0);
        for (int i = ty; i <= n; i += 16)
            for (int j = tx; j <= i; j += 16) {
                double sum = 0.0;
                for (int rr = 0; rr < R; ++rr)
                    if (rok[rr]) sum += (rwr[rr] * Gt[rr * n1 + i]) * Gt[rr * n1 + j];
                M[lsq_tri(i, j)] += sum;
            }
        for (int rr = 0; rr < R; ++rr) used += rok[rr];
        __syncthreads();
    }

    // ---- regularisation: alpha D^T Q D + lambda I on the band, -alpha D^T Q D x0 on row n; misfit and roughness at x0
    const double alpha = A.alpha, lam = A.lam[s];
    double misfit = 0.0, rough = 0.0;
    if (tid == 0) {
        misfit = M[lsq_tri(n, n)];
        for (int j = 0; j + 1 < n; ++j) { const double d = x0[j + 1] - x0[j]; rough += qw[j] * d * d; }
        sh_flag = used == 0 ? 1 : 0;
    }
    for (int j = tid; j < n; j += 256) {
        const double qa = j > 0 ? qw[j - 1] : 0.0, qb = j + 1 < n ? qw[j] : 0.0;
        const double da = j > 0 ? x0[j] - x0[j - 1] : 0.0, db = j + 1 < n ? x0[j + 1] - x0[j] : 0.0;
        M[lsq_tri(j, j)] += alpha * (qa + qb) + lam;
        if (j + 1 < n) M[lsq_tri(j + 1, j)] -= alpha * qb;
        M[lsq_tri(n, j)] -= alpha * (qa * da - qb * db);
    }
    __syncthreads();
    int flag = sh_flag;

    // ---- Cholesky factorisation of the columns 0..n-1 over the rows 0..n (row n becomes y = L^-1 g), then L^T delta = y
    if (flag == 0) {
        for (int k = 0; k < n; ++k) {
            const double d = M[lsq_tri(k, k)];                             // the same value in every lane: a uniform exit
            if (!(d > 0.0) || !lsq_finite(d)) { flag = 2; break; }
            const double l = sqrt(d);
            for (int i = k + tid; i <= n; i += 256) {
                if (i == k) dg[k] = l;
                else { const double v = M[lsq_tri(i, k)] / l; M[lsq_tri(i, k)] = v; cv[i] = v; }
            }
            __syncthreads();
            for (int i = k + 1 + ty; i <= n; i += 16) {
                const double ci = cv[i];
                for (int j = k + 1 + tx; j <= i; j += 16) M[lsq_tri(i, j)] -= ci * cv[j];
            }
            __syncthreads();
        }
    }
    if (flag == 0) {
        for (int j = tid; j < n; j += 256) cv[j] = M[lsq_tri(n, j)];
        __syncthreads();
        for (int k = n - 1; k >= 0; --k) {
            const double dk = cv[k] / dg[k];
            if (tid < k) cv[tid] -= M[lsq_tri(k, tid)] * dk;
            if (tid == k) { dl[k] = dk; if (!lsq_finite(dk)) sh_flag = 2; }
            __syncthreads();
        }
        flag = sh_flag;                                                    // (a step that overflowed counts as a failed pivot)
    }

    // ---- the objective the linear model predicts at x0 + delta: sum W (res - G delta)^2 + alpha roughness(x0 + delta)
    double pred = misfit + alpha * rough;
    if (flag == 0) {
        pred = 0.0;
        for (int r0 = 0; r0 < A.N; r0 += R) {
            stage(r0);
            if (tid < R) {
                double t = 0.0;
                if (rok[tid]) {
                    t = Gt[tid * n1 + n];
                    for (int j = 0; j < n; ++j) t -= Gt[tid * n1 + j] * dl[j];
                }
                rt[tid] = rwr[tid] * t * t;
            }
            __syncthreads();
            if (tid == 0)
                for (int rr = 0; rr < R; ++rr) pred += rt[rr];
        }
        if (tid == 0) {
            double r2 = 0.0;
            for (int j = 0; j + 1 < n; ++j) { const double d = (x0[j + 1] + dl[j + 1]) - (x0[j] + dl[j]); r2 += qw[j] * d * d; }
            pred += alpha * r2;
        }
    }

    for (int i = tid; i < Lmax; i += 256) delta[i] = (flag == 0 && pos[i] >= 0) ? dl[pos[i]] : 0.0;
    if (tid == 0) {
        A.stats[3 * (size_t)s] = misfit; A.stats[3 * (size_t)s + 1] = rough; A.stats[3 * (size_t)s + 2] = pred;
        A.info[3 * (size_t)s] = used; A.info[3 * (size_t)s + 1] = A.N - used; A.info[3 * (size_t)s + 2] = flag;
    }
}

// One workgroup per stack.  The dynamic-LDS limit of the kernel is raised when a launch needs more than any before it on
// the device (as launch_phase_g does): a caller that captures a graph makes its first call outside the capture.
hipError_t launch_lsq_step(hipStream_t s, const LsqArgs &a)
{
    constexpr int MAXDEV = 64;
    static std::atomic<size_t> lds_set[MAXDEV];
    const size_t lds = lsq_lds_bytes(a.nmax);
    int dev = 0;
    (void)hipGetDevice(&dev);
    const int di = (dev >= 0 && dev < MAXDEV) ? dev : 0;
    if (lds > lds_set[di].load(std::memory_order_acquire) || dev != di) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(surfdisp_lsq_step_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        size_t cur = lds_set[di].load(std::memory_order_relaxed);
        while (lds > cur && !lds_set[di].compare_exchange_weak(cur, lds, std::memory_order_release)) {}
    }
    hipLaunchKernelGGL(surfdisp_lsq_step_kernel, dim3((unsigned)a.B), dim3(256), lds, s, a);
    return hipGetLastError();
}

}  // namespace sd
