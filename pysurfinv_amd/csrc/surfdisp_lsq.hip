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
// The second kernel of this file, surfdisp_lsq_resolution_kernel (section (6e)), turns the same matrix into the posterior
// covariance and the resolution matrix; the two share the row rules through lsq_stage_rows.
// THICKNESS MODES (section (6h)): both kernels and lsq_stage_rows are templates on MODES.  The <false> instantiations are the
// kernels of (6d) / (6e) as they were; the <true> ones carry K = 1..8 more unknowns behind the n Vs unknowns (nu = n + K): mode
// k's column of a row is sg * sum_i part_h[i] T_k[i] over the layers above the half space, T [K][Lmax] staged once in LDS
// behind the staged rows, one 16-lane group per (row, mode) reading consecutive layers of both.  D acts on the Vs unknowns
// only; mode k takes lam ms_k + beta_k on its diagonal and -beta_k y_k on the right-hand side.
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

// The LDS arrays of the SD_LSQ_TILE_ROWS rows staged at a time (each kernel declares its own and hands them over)
struct LsqRows {
    const float **rkb, **rka, **rkr;   // the row's partial arrays at its (stack, period), or nullptr
    const float **rkh;                 // ... and its thickness kernel dcdh (the MODES kernels only)
    double *rwr, *rsg;                 // weight w_r / uncer_r^2 (0 for a row that is not used), sign of a source-5 row
    int *rok, *rbad;                   // the row is used; a non-finite entry was found in it
};

// Stage the rows r0 .. r0 + SD_LSQ_TILE_ROWS - 1 of stack s into Gt [R][n + 1] (column n = residual): validity, weight, sign,
// effective Jacobian row, NaN-row drop - the row rules of include/surfdisp.h section (6d), for the step and the resolution
// kernel alike.  Called by the whole workgroup; ends on a barrier.  MODES: K more columns behind the n of the free layers -
// Tm [K][Lmax] the stack's mode shapes in LDS, nlm = nlay - 1 the layers that have a thickness - and two more reasons to drop
// a row: its source has no part_h array, or one of its mode columns is not finite (section (6h)).
template <bool MODES>
__device__ __forceinline__ void lsq_stage_rows(const LsqArgs &A, const LsqRows &W, int s, size_t ob, int r0, int n, const int *fidx,
                                               const double *ps, const double *qs, double *Gt, int Kin = 0, int nlm = 0,
                                               const double *Tm = nullptr)
{
    constexpr int R = SD_LSQ_TILE_ROWS;
    const int K = MODES ? Kin : 0;
    const int tid = threadIdx.x, Lmax = A.Lmax, nu = n + K, n1 = nu + 1;
    if (tid < R) {
        const int r = r0 + tid;
        int ok = 0;
        double wr = 0.0, sg = 1.0, res = 0.0;
        const float *kb = nullptr, *ka = nullptr, *kr = nullptr, *kh = nullptr;
        if (r < A.N) {
            const int src = A.cols[2 * r], idx = A.cols[2 * r + 1];
            const int sa = src == 5 ? 4 : src;                         // sources 4 and 5 read the same solve's chi
            const float *pp = nullptr;
            long pst = 0;
#pragma unroll
            for (int k = 0; k < 5; ++k)
                if (k == sa) {
                    pp = A.pred[k]; pst = A.pstride[k]; kb = A.part[3 * k]; ka = A.part[3 * k + 1]; kr = A.part[3 * k + 2];
                    if constexpr (MODES) kh = A.part_h[k];
                }
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
                if constexpr (MODES) solved = solved && kh != nullptr;     // the row names a missing thickness array
                if (solved) {
                    ok = 1;
                    wr = A.weights[r] / (sgm * sgm);
                    res = o - v;
                    const size_t off = ((size_t)s * P + idx) * Lmax;
                    kb = kb ? kb + off : nullptr; ka = ka ? ka + off : nullptr; kr = kr ? kr + off : nullptr;
                    if constexpr (MODES) kh += off;
                }
            }
        }
        W.rok[tid] = ok; W.rbad[tid] = 0; W.rwr[tid] = wr; W.rsg[tid] = sg;
        W.rkb[tid] = kb; W.rka[tid] = ka; W.rkr[tid] = kr;
        if constexpr (MODES) W.rkh[tid] = kh;
        Gt[tid * n1 + nu] = res;
    }
    __syncthreads();
    for (int t = tid; t < R * n; t += 256) {
        const int rr = t / n, j = t - rr * n;
        if (W.rok[rr]) {
            const int i = fidx[j];
            const float *kb = W.rkb[rr], *ka = W.rka[rr], *kr = W.rkr[rr];
            double g = kb ? (double)kb[i] : 0.0;
            if (ka && ps[j] != 0.0) g += ps[j] * (double)ka[i];
            if (kr && qs[j] != 0.0) g += qs[j] * (double)kr[i];
            g *= W.rsg[rr];
            if (!lsq_finite(g)) W.rbad[rr] = 1;                           // a NaN row of a failed unit: dropped
            Gt[rr * n1 + j] = g;
        }
    }
    if constexpr (MODES) {                                                 // one 16-lane group per (row, mode): consecutive layers
        const int tx = tid & 15, ty = tid >> 4;
        for (int p = ty; p < R * K; p += 16) {
            const int rr = p / K, k = p - rr * K;
            const bool on = W.rok[rr] != 0;
            const float *kh = W.rkh[rr];
            const double *T = Tm + k * Lmax;
            double sum = 0.0;
            if (on)
                for (int i = tx; i < nlm; i += 16) sum += (double)kh[i] * T[i];
            sum += __shfl_xor(sum, 8, 16); sum += __shfl_xor(sum, 4, 16); sum += __shfl_xor(sum, 2, 16); sum += __shfl_xor(sum, 1, 16);
            if (on && tx == 0) {
                sum *= W.rsg[rr];
                if (!lsq_finite(sum)) W.rbad[rr] = 1;                      // a NaN row of the thickness entry: dropped
                Gt[rr * n1 + n + k] = sum;
            }
        }
    }
    __syncthreads();
    if (tid < R) {
        const int fin = W.rok[tid] && !W.rbad[tid];
        W.rok[tid] = fin;
        if (!fin) W.rwr[tid] = 0.0;
    }
    __syncthreads();
}

// MODES: the step of section (6h).  n stays the number of Vs unknowns, nu = n + K the number of unknowns; row nu of M is the
// right-hand side.  The dynamic LDS holds M and Gt for nmax + K unknowns and, behind them, T [K][Lmax].
template <bool MODES>
__global__ __launch_bounds__(256) void surfdisp_lsq_step_kernel(LsqArgs A)
{
    constexpr int R = SD_LSQ_TILE_ROWS, NF = SD_LSQ_MAX_FREE + (MODES ? SD_LSQ_MAX_MODES : 0) + 1;
    constexpr int NK = MODES ? SD_LSQ_MAX_MODES : 1, RH = MODES ? R : 1;
    extern __shared__ double lsq_smem[];
    __shared__ double x0[NF], ps[NF], qs[NF], qw[NF], cv[NF], dg[NF], dl[NF];
    __shared__ int fidx[NF], pos[SURFDISP_NLAY_MAX];
    __shared__ const float *rkb[R], *rka[R], *rkr[R], *rkh[RH];
    __shared__ double rwr[R], rsg[R], rt[R];
    __shared__ double mdiag[NK], mbeta[NK], my[NK];    // lam ms_k + beta_k, beta_k, y_k of the modes
    __shared__ int rok[R], rbad[R];
    __shared__ int sh_n, sh_over, sh_flag;

    const int s = blockIdx.x, tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int Lmax = A.Lmax;
    const int K = MODES ? A.K : 0;
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
        if constexpr (MODES)
            if (tid < K) A.delta_y[(size_t)s * K + tid] = 0.0;
        if (tid == 0) {
            A.stats[3 * (size_t)s] = 0.0; A.stats[3 * (size_t)s + 1] = 0.0; A.stats[3 * (size_t)s + 2] = 0.0;
            A.info[3 * (size_t)s] = 0; A.info[3 * (size_t)s + 1] = A.N; A.info[3 * (size_t)s + 2] = 3;
        }
        return;
    }
    const int nu = n + K, n1 = nu + 1, nm = A.nmax + K;
    double *M = lsq_smem;                            // packed lower triangle of the (nu + 1) x (nu + 1) augmented matrix
    double *Gt = lsq_smem + (size_t)(nm + 1) * (nm + 2) / 2;           // [R][n1]: staged rows, column nu = residual
    double *Tm = Gt + (size_t)R * (nm + 1);          // MODES: [K][Lmax], the mode shapes of this stack
    const int tot = n1 * (n1 + 1) / 2;

    if constexpr (MODES) {
        const size_t mo = A.modes_per_stack ? (size_t)s * K : 0;
        const double *Tg = A.modes + mo * Lmax;
        for (int t = tid; t < K * Lmax; t += 256) Tm[t] = Tg[t];
        if (tid < K) {
            const double beta = A.mode_prior ? A.mode_prior[mo + tid] : 0.0;
            mbeta[tid] = beta;
            mdiag[tid] = A.lam[s] * A.mode_scale[mo + tid] + beta;
            my[tid] = A.mode_y ? A.mode_y[(size_t)s * K + tid] : 0.0;
        }
    }
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

    const LsqRows rows{rkb, rka, rkr, rkh, rwr, rsg, rok, rbad};
    auto stage = [&](int r0) { lsq_stage_rows<MODES>(A, rows, s, ob, r0, n, fidx, ps, qs, Gt, K, nl - 1, Tm); };

    // ---- [G | res]^T W [G | res] into M
    int used = 0;                                                          // (thread 0's copy counts)
    for (int r0 = 0; r0 < A.N; r0 += R) {
        stage(r0);
        for (int i = ty; i <= nu; i += 16)
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
    double misfit = 0.0, rough = 0.0, prior = 0.0;                         // prior: sum beta_k y_k^2 (MODES)
    if (tid == 0) {
        misfit = M[lsq_tri(nu, nu)];
        for (int j = 0; j + 1 < n; ++j) { const double d = x0[j + 1] - x0[j]; rough += qw[j] * d * d; }
        if constexpr (MODES)
            for (int k = 0; k < K; ++k) prior += mbeta[k] * my[k] * my[k];
        sh_flag = used == 0 ? 1 : 0;
    }
    for (int j = tid; j < n; j += 256) {
        const double qa = j > 0 ? qw[j - 1] : 0.0, qb = j + 1 < n ? qw[j] : 0.0;
        const double da = j > 0 ? x0[j] - x0[j - 1] : 0.0, db = j + 1 < n ? x0[j + 1] - x0[j] : 0.0;
        M[lsq_tri(j, j)] += alpha * (qa + qb) + lam;
        if (j + 1 < n) M[lsq_tri(j + 1, j)] -= alpha * qb;
        M[lsq_tri(nu, j)] -= alpha * (qa * da - qb * db);
    }
    if constexpr (MODES)
        if (tid < K) {                                                     // lam ms_k + beta_k on the diagonal, -beta_k y_k on the right
            M[lsq_tri(n + tid, n + tid)] += mdiag[tid];
            M[lsq_tri(nu, n + tid)] -= mbeta[tid] * my[tid];
        }
    __syncthreads();
    int flag = sh_flag;

    // ---- Cholesky factorisation of the columns 0..nu-1 over the rows 0..nu (row nu becomes y = L^-1 g), then L^T delta = y
    if (flag == 0) {
        for (int k = 0; k < nu; ++k) {
            const double d = M[lsq_tri(k, k)];                             // the same value in every lane: a uniform exit
            if (!(d > 0.0) || !lsq_finite(d)) { flag = 2; break; }
            const double l = sqrt(d);
            for (int i = k + tid; i <= nu; i += 256) {
                if (i == k) dg[k] = l;
                else { const double v = M[lsq_tri(i, k)] / l; M[lsq_tri(i, k)] = v; cv[i] = v; }
            }
            __syncthreads();
            for (int i = k + 1 + ty; i <= nu; i += 16) {
                const double ci = cv[i];
                for (int j = k + 1 + tx; j <= i; j += 16) M[lsq_tri(i, j)] -= ci * cv[j];
            }
            __syncthreads();
        }
    }
    if (flag == 0) {
        for (int j = tid; j < nu; j += 256) cv[j] = M[lsq_tri(nu, j)];
        __syncthreads();
        for (int k = nu - 1; k >= 0; --k) {
            const double dk = cv[k] / dg[k];
            if (tid < k) cv[tid] -= M[lsq_tri(k, tid)] * dk;
            if (tid == k) { dl[k] = dk; if (!lsq_finite(dk)) sh_flag = 2; }
            __syncthreads();
        }
        flag = sh_flag;                                                    // (a step that overflowed counts as a failed pivot)
    }

    // ---- the objective the linear model predicts at x0 + delta: sum W (res - G delta)^2 + alpha roughness(x0 + delta)
    double pred = misfit + alpha * rough;
    if constexpr (MODES) pred += prior;
    if (flag == 0) {
        pred = 0.0;
        for (int r0 = 0; r0 < A.N; r0 += R) {
            stage(r0);
            if (tid < R) {
                double t = 0.0;
                if (rok[tid]) {
                    t = Gt[tid * n1 + nu];
                    for (int j = 0; j < nu; ++j) t -= Gt[tid * n1 + j] * dl[j];
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
            if constexpr (MODES)
                for (int k = 0; k < K; ++k) { const double y = my[k] + dl[n + k]; pred += mbeta[k] * y * y; }
        }
    }

    for (int i = tid; i < Lmax; i += 256) delta[i] = (flag == 0 && pos[i] >= 0) ? dl[pos[i]] : 0.0;
    if constexpr (MODES)
        if (tid < K) A.delta_y[(size_t)s * K + tid] = flag == 0 ? dl[n + tid] : 0.0;
    if (tid == 0) {
        A.stats[3 * (size_t)s] = misfit; A.stats[3 * (size_t)s + 1] = rough; A.stats[3 * (size_t)s + 2] = pred;
        A.info[3 * (size_t)s] = used; A.info[3 * (size_t)s + 1] = A.N - used; A.info[3 * (size_t)s + 2] = flag;
    }
}

size_t lsq_resolution_lds_bytes(int nmax)
{
    return ((size_t)nmax * (nmax + 1) / 2 + (size_t)SD_LSQ_TILE_ROWS * (nmax + 1)) * sizeof(double);
}

// Posterior covariance and resolution of the same damped, smoothed problem (include/surfdisp.h section (6e); the host statement
// is pysurfinv_amd.linearized.lsq_resolution_reference).  One workgroup of 256 lanes per stack; the rows are staged by
// lsq_stage_rows, so the unknowns, weights and dropped rows are those of the step.  In the packed lower triangle M of LDS:
//   1. A = G^T W G + alpha D^T Q D + lam I is accumulated and factorised A = L L^T as in the step kernel (the pivots go to dg
//      as 1 / l, log det A = sum of log(pivot) on the way);
//   2. L is inverted in place, column j = n-2 .. 0: from T L = I, T_ij = -(sum_{k=j+1..i} T_ik L_kj) / L_jj - row i of T is
//      read along the packed row (16 lanes per row, 16 consecutive doubles at a time), the column L_.j from a contiguous copy
//      made one column ahead (cv, two buffers: one barrier per column);
//   3. C = T^T T overwrites T row by row, i ascending (row i of C needs the rows k >= i of T only): a lane owns a column j,
//      256 / W rows in flight (W = 16..128 >= n), C_ij = sum_{k>=i} T_ki T_kj with T_.i from a contiguous copy and T_kj
//      consecutive across the lanes.  Only the lower triangle exists, so cov is symmetric by construction;
//   4. the resolution needs no second matrix: H = A - alpha D^T Q D - lam I, so R = C H = I - C (alpha D^T Q D + lam I), three
//      entries of C per entry of R, O(n^2).  Its error is a few ulp of 1 in absolute terms whatever the damping (the product
//      C H loses cond(A) eps when the damping is weak, this form loses the relative accuracy of entries below ~1e-8 when it
//      is strong); H is not held, which keeps the launch at half the LDS.  diag(C H C) = sum_k R_ik C_ik falls out of the same
//      pass by a 16-lane reduction.
// Steps 1-3 are n^3 / 2 FMAs after the N n^2 / 2 of the accumulation.  The strided column reads (once per column / row
// block) and the upper half of C's rows in step 4 are the only LDS accesses that are not consecutive across lanes.
// MODES (section (6h)): n stays the number of Vs unknowns, nu = n + K the size of the matrices, no = nfree_max + K the rows of
// cov and res; the regularisation of unknown j >= n is the diagonal entry lam ms_k + beta_k alone.
template <bool MODES>
__global__ __launch_bounds__(256) void surfdisp_lsq_resolution_kernel(LsqArgs A)
{
    constexpr int R = SD_LSQ_TILE_ROWS, NM = SD_LSQ_MAX_FREE + (MODES ? SD_LSQ_MAX_MODES : 0), NF = NM + 1;
    constexpr int NK = MODES ? SD_LSQ_MAX_MODES : 1, RH = MODES ? R : 1;
    extern __shared__ double lsq_smem[];
    __shared__ double ps[NF], qs[NF], qw[NF], dg[NF], cv[2 * NM];
    __shared__ double ocd[NM], ord[NM], odd[NM];                           // C_jj, R_jj, (C H C)_jj
    __shared__ int fidx[NF], pos[SURFDISP_NLAY_MAX];
    __shared__ const float *rkb[R], *rka[R], *rkr[R], *rkh[RH];
    __shared__ double rwr[R], rsg[R];
    __shared__ double mdiag[NK];                                           // lam ms_k + beta_k of the modes
    __shared__ int rok[R], rbad[R];
    __shared__ int sh_n, sh_over, sh_flag;

    const int s = blockIdx.x, tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int Lmax = A.Lmax, nmax = A.nmax;
    const int K = MODES ? A.K : 0, no = nmax + K;
    int nl = A.nlay ? A.nlay[s] : Lmax;
    nl = nl < 0 ? 0 : (nl > Lmax ? Lmax : nl);
    const size_t ob = A.obs_per_stack ? (size_t)s * A.N : 0;

    // ---- the free layers of this stack, in order (as the step kernel)
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
            if (f && k < nmax) { fidx[k] = i; pos[i] = k; }
            cnt += __popcll(m);
        }
        if (tid == 0) { sh_n = cnt < nmax ? cnt : nmax; sh_over = cnt > nmax ? 1 : 0; sh_flag = 0; }
    }
    __syncthreads();
    const int n = sh_n;
    double *cov = A.cov ? A.cov + (size_t)s * no * no : nullptr;
    double *res = A.res ? A.res + (size_t)s * no * no : nullptr;
    double *o_post = A.sigma_post + (size_t)s * Lmax, *o_data = A.sigma_data + (size_t)s * Lmax, *o_rd = A.rdiag + (size_t)s * Lmax;
    // every output of a stack that is not solved is zeros
    auto refuse = [&](int used, int flag) {
        for (int t = tid; t < no * no; t += 256) {
            if (cov) cov[t] = 0.0;
            if (res) res[t] = 0.0;
        }
        for (int i = tid; i < Lmax; i += 256) { o_post[i] = 0.0; o_data[i] = 0.0; o_rd[i] = 0.0; }
        if constexpr (MODES)
            if (tid < K) { A.sigma_post_y[(size_t)s * K + tid] = 0.0; A.sigma_data_y[(size_t)s * K + tid] = 0.0; A.rdiag_y[(size_t)s * K + tid] = 0.0; }
        if (tid == 0) {
            A.stats[2 * (size_t)s] = 0.0; A.stats[2 * (size_t)s + 1] = 0.0;
            A.info[3 * (size_t)s] = used; A.info[3 * (size_t)s + 1] = A.N - used; A.info[3 * (size_t)s + 2] = flag;
        }
    };
    if (sh_over) { refuse(0, 3); return; }           // more free layers than the caller sized the launch for
    const int nu = n + K, n1 = nu + 1;
    double *M = lsq_smem;                            // packed lower triangle, nu x nu: A, then L, then T = L^-1, then C
    double *Gt = lsq_smem + (size_t)no * (no + 1) / 2;                // [R][n1]: staged rows (column nu, the residual, is not read)
    double *Tm = Gt + (size_t)R * (no + 1);          // MODES: [K][Lmax], the mode shapes of this stack
    const int tot = nu * (nu + 1) / 2;

    if constexpr (MODES) {
        const size_t mo = A.modes_per_stack ? (size_t)s * K : 0;
        const double *Tg = A.modes + mo * Lmax;
        for (int t = tid; t < K * Lmax; t += 256) Tm[t] = Tg[t];
        if (tid < K) mdiag[tid] = A.lam[s] * A.mode_scale[mo + tid] + (A.mode_prior ? A.mode_prior[mo + tid] : 0.0);
    }
    {
        const double *vps = A.vp_slope ? A.vp_slope + (A.slope_per_stack ? (size_t)s * Lmax : 0) : nullptr;
        const double *rhs = A.rho_slope ? A.rho_slope + (A.slope_per_stack ? (size_t)s * Lmax : 0) : nullptr;
        const double *Q = A.Q ? A.Q + (A.q_per_stack ? (size_t)s * (Lmax - 1) : 0) : nullptr;
        for (int j = tid; j < n; j += 256) {
            const int i = fidx[j];
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

    // ---- G^T W G into M
    const LsqRows rows{rkb, rka, rkr, rkh, rwr, rsg, rok, rbad};
    int used = 0;                                                          // (the same count in every lane)
    for (int r0 = 0; r0 < A.N; r0 += R) {
        lsq_stage_rows<MODES>(A, rows, s, ob, r0, n, fidx, ps, qs, Gt, K, nl - 1, Tm);
        for (int i = ty; i < nu; i += 16)
            for (int j = tx; j <= i; j += 16) {
                double sum = 0.0;
                for (int rr = 0; rr < R; ++rr)
                    if (rok[rr]) sum += (rwr[rr] * Gt[rr * n1 + i]) * Gt[rr * n1 + j];
                M[lsq_tri(i, j)] += sum;
            }
        for (int rr = 0; rr < R; ++rr) used += rok[rr];
        __syncthreads();
    }
    if (used == 0) { refuse(0, 1); return; }

    // ---- A = G^T W G + alpha D^T Q D + lam I
    const double alpha = A.alpha, lam = A.lam[s];
    for (int j = tid; j < n; j += 256) {
        const double qa = j > 0 ? qw[j - 1] : 0.0, qb = j + 1 < n ? qw[j] : 0.0;
        M[lsq_tri(j, j)] += alpha * (qa + qb) + lam;
        if (j + 1 < n) M[lsq_tri(j + 1, j)] -= alpha * qb;
    }
    if constexpr (MODES)
        if (tid < K) M[lsq_tri(n + tid, n + tid)] += mdiag[tid];
    __syncthreads();

    // ---- 1. Cholesky factorisation in place (the diagonal of M keeps the pivots; dg = 1 / l)
    int flag = 0;
    double logdet = 0.0;                                                   // (thread 0's copy counts)
    for (int k = 0; k < nu; ++k) {
        const double d = M[lsq_tri(k, k)];                                 // the same value in every lane: a uniform exit
        if (!(d > 0.0) || !lsq_finite(d)) { flag = 2; break; }
        const double l = sqrt(d);
        if (tid == 0) { dg[k] = 1.0 / l; logdet += log(d); }
        for (int i = k + 1 + tid; i < nu; i += 256) { const double v = M[lsq_tri(i, k)] / l; M[lsq_tri(i, k)] = v; cv[i] = v; }
        __syncthreads();
        for (int i = k + 1 + ty; i < nu; i += 16) {
            const double ci = cv[i];
            for (int j = k + 1 + tx; j <= i; j += 16) M[lsq_tri(i, j)] -= ci * cv[j];
        }
        __syncthreads();
    }
    if (flag != 0) { refuse(used, flag); return; }

    // ---- 2. T = L^-1 in place, column by column from the right
    for (int i = tid; i < nu; i += 256) M[lsq_tri(i, i)] = dg[i];
    if (tid == 0 && nu >= 2) cv[((nu - 2) & 1) * NM + nu - 1] = M[lsq_tri(nu - 1, nu - 2)];
    __syncthreads();
    for (int j = nu - 2; j >= 0; --j) {
        const double *c = cv + (j & 1) * NM;                               // c[k] = L_kj, k > j
        const double tjj = dg[j];
        for (int i = j + 1 + ty; i < nu; i += 16) {
            const double *row = M + lsq_tri(i, 0);
            double sum = 0.0;
            for (int k = j + 1 + tx; k <= i; k += 16) sum += row[k] * c[k];
            sum += __shfl_xor(sum, 8, 16); sum += __shfl_xor(sum, 4, 16); sum += __shfl_xor(sum, 2, 16); sum += __shfl_xor(sum, 1, 16);
            if (tx == 0) M[lsq_tri(i, j)] = -sum * tjj;
        }
        if (j > 0)                                                         // the next column of L, untouched so far
            for (int i = j + tid; i < nu; i += 256) cv[((j - 1) & 1) * NM + i] = M[lsq_tri(i, j - 1)];
        __syncthreads();
    }

    // ---- 3. C = T^T T in place, RB rows at a time: lane (a, j) forms C_{i0+a, j}
    {
        const int W = nu <= 16 ? 16 : (nu <= 32 ? 32 : (nu <= 64 ? 64 : (!MODES || nu <= 128 ? 128 : 256))), RB = 256 / W;
        const int a = tid / W, j = tid - a * W;
        for (int i0 = 0; i0 < nu; i0 += RB) {
            for (int t = tid; t < RB * W; t += 256) {                      // cv[a][k] = T_{k, i0+a}, k >= i0 + a
                const int aa = t / W, k = t - aa * W, i = i0 + aa;
                if (i < nu && k >= i && k < nu) cv[aa * W + k] = M[lsq_tri(k, i)];
            }
            __syncthreads();
            const int i = i0 + a;
            double sum = 0.0;
            if (i < nu && j <= i)
                for (int k = i; k < nu; ++k) sum += cv[a * W + k] * M[lsq_tri(k, j)];
            __syncthreads();
            if (i < nu && j <= i) M[lsq_tri(i, j)] = sum;
        }
        __syncthreads();
    }

    // ---- 4. cov, res = I - C (alpha D^T Q D + lam I), and the diagonals (MODES: lam ms_k + beta_k in place of lam, no D)
    auto Cs = [&](int i, int j) { return i >= j ? M[lsq_tri(i, j)] : M[lsq_tri(j, i)]; };
    int bad = 0;
    for (int i = ty; i < no; i += 16) {
        double part = 0.0;
        for (int j = tx; j < no; j += 16) {
            double c = 0.0, r = 0.0;
            if (i < nu && j < nu) {
                if (!MODES || j < n) {
                    const double qa = j > 0 ? qw[j - 1] : 0.0, qb = j + 1 < n ? qw[j] : 0.0;
                    c = Cs(i, j);
                    double sc = (qa + qb) * c;                             // (C D^T Q D)_ij
                    if (j > 0) sc -= qa * Cs(i, j - 1);
                    if (j + 1 < n) sc -= qb * Cs(i, j + 1);
                    r = ((i == j ? 1.0 : 0.0) - lam * c) - alpha * sc;
                } else {
                    c = Cs(i, j);
                    r = (i == j ? 1.0 : 0.0) - mdiag[j - n] * c;
                }
                part += r * c;
                if (!lsq_finite(c) || !lsq_finite(r)) bad = 1;
                if (i == j) { ocd[i] = c; ord[i] = r; }
            }
            if (cov) cov[(size_t)i * no + j] = c;
            if (res) res[(size_t)i * no + j] = r;
        }
        part += __shfl_xor(part, 8, 16); part += __shfl_xor(part, 4, 16); part += __shfl_xor(part, 2, 16); part += __shfl_xor(part, 1, 16);
        if (tx == 0 && i < nu) { odd[i] = part; if (!lsq_finite(part)) bad = 1; }
    }
    if (bad) sh_flag = 2;
    __syncthreads();
    if (sh_flag != 0) { refuse(used, 2); return; }                         // an inverse that overflowed counts as a failed pivot
    for (int i = tid; i < Lmax; i += 256) {
        const int j = pos[i];
        o_post[i] = j >= 0 ? sqrt(ocd[j]) : 0.0;
        o_data[i] = j >= 0 ? sqrt(odd[j] > 0.0 ? odd[j] : 0.0) : 0.0;
        o_rd[i] = j >= 0 ? ord[j] : 0.0;
    }
    if constexpr (MODES)
        if (tid < K) {
            const int j = n + tid;
            A.sigma_post_y[(size_t)s * K + tid] = sqrt(ocd[j]);
            A.sigma_data_y[(size_t)s * K + tid] = sqrt(odd[j] > 0.0 ? odd[j] : 0.0);
            A.rdiag_y[(size_t)s * K + tid] = ord[j];
        }
    if (tid == 0) {
        double dof = 0.0;
        for (int j = 0; j < nu; ++j) dof += ord[j];
        A.stats[2 * (size_t)s] = dof; A.stats[2 * (size_t)s + 1] = logdet;
        A.info[3 * (size_t)s] = used; A.info[3 * (size_t)s + 1] = A.N - used; A.info[3 * (size_t)s + 2] = 0;
    }
}

// One workgroup per stack.  The dynamic-LDS limit of a kernel is raised when a launch needs more than any before it on
// the device (as launch_phase_g does): a caller that captures a graph makes its first call outside the capture.
template <typename K>
static hipError_t lsq_launch(K kernel, std::atomic<size_t> *lds_set, size_t lds, hipStream_t s, const LsqArgs &a)
{
    constexpr int MAXDEV = 64;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const int di = (dev >= 0 && dev < MAXDEV) ? dev : 0;
    if (lds > lds_set[di].load(std::memory_order_acquire) || dev != di) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        size_t cur = lds_set[di].load(std::memory_order_relaxed);
        while (lds > cur && !lds_set[di].compare_exchange_weak(cur, lds, std::memory_order_release)) {}
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)a.B), dim3(256), lds, s, a);
    return hipGetLastError();
}

// K = 0 is the kernel of (6d) / (6e) itself; K > 0 its MODES instantiation, sized for nmax + K unknowns and T [K][Lmax].
hipError_t launch_lsq_step(hipStream_t s, const LsqArgs &a)
{
    static std::atomic<size_t> lds_set[64], lds_set_modes[64];
    if (a.K > 0)
        return lsq_launch(surfdisp_lsq_step_kernel<true>, lds_set_modes,
                          lsq_lds_bytes(a.nmax + a.K) + (size_t)a.K * a.Lmax * sizeof(double), s, a);
    return lsq_launch(surfdisp_lsq_step_kernel<false>, lds_set, lsq_lds_bytes(a.nmax), s, a);
}

hipError_t launch_lsq_resolution(hipStream_t s, const LsqArgs &a)
{
    static std::atomic<size_t> lds_set[64], lds_set_modes[64];
    if (a.K > 0)
        return lsq_launch(surfdisp_lsq_resolution_kernel<true>, lds_set_modes,
                          lsq_resolution_lds_bytes(a.nmax + a.K) + (size_t)a.K * a.Lmax * sizeof(double), s, a);
    return lsq_launch(surfdisp_lsq_resolution_kernel<false>, lds_set, lsq_resolution_lds_bytes(a.nmax), s, a);
}

}  // namespace sd
