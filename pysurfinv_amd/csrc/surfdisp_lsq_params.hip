// surfdisp_lsq_params.hip -- linearised inversion in the SAMPLER's parameters (include/surfdisp.h section (6i)): the Jacobian of the
// params -> stack map of surfdisp_layers.hip, and one damped least-squares step of the parameters themselves, fed by the analytic
// sensitivity kernels of (5b)/(5c) and the thickness kernels of (5g)/(5h).  The host statements are
// pysurfinv_amd.paramlsq.jacobian_reference and param_lsq_reference.
//
// K1 surfdisp_params_jacobian_kernel: one thread per (chain, output layer, unknown j), j fastest - the stores of jac [C][4][L][Nu]
//    are consecutive across lanes.  Each thread evaluates its layer as a dual number for its one j (surfdisp_layers_dual.h): no
//    array over j in registers.
// K2 surfdisp_lsq_step_params_kernel: one workgroup of 256 lanes per stack, after surfdisp_lsq_step_kernel (surfdisp_lsq.hip): the
//    augmented matrix [G | res]^T W [G | res] over the n free unknowns is accumulated in fp64 into a packed lower triangle of LDS, 16
//    data rows at a time, then damped, factorised by a right-looking Cholesky over n + 1 rows, and back-substituted.  G is never
//    stored beyond the 16 staged rows: row r's column j is the chain rule
//        G[r,j] = sg_r (sum_{i<nlay} K_b[i] jac[vs][i][j] + K_a[i] jac[vp][i][j] + K_rho[i] jac[rho][i][j] + sum_{i<nlay-1} K_h[i] jac[h][i][j])
//    summed in fp64, layers ascending, a term whose jac entry is exactly 0 skipped (a water layer's NaN d/dVs meets a zero there).
//    Lane mapping: the four fp32 kernel rows of the 16 staged data rows are brought into LDS 64 layers at a time, consecutive lanes
//    reading consecutive layers (coalesced); then lane (row, j) walks the chunk, consecutive lanes reading consecutive j of one jac
//    row from global memory (coalesced, Nu doubles per layer and quantity) and one LDS value per data row (a broadcast).
//    With cov / sigma wanted the factor is inverted in place and C = L^-T L^-1 formed in the same triangle, as
//    surfdisp_lsq_resolution_kernel does.
// LDS, all static, whatever Nu: triangle 65 * 66 / 2 doubles (17 160 B) + staged rows 16 x 65 doubles (8 320 B) + kernel chunk
// 16 x 4 x 64 floats (16 384 B) + 256 doubles of column copies (2 048 B) + per-unknown and per-row vectors (~4 KB): 48 112 B.
// Everything indexed by unknown or row lives in LDS: no private arrays, no scratch (tests/test_isa_guard.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "surfdisp_internal.h"
#include "surfdisp_layers_dual.h"

namespace sd {

__global__ __launch_bounds__(256) void surfdisp_params_jacobian_kernel(ParamsJacArgs A)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int L = A.L, Nu = A.Nu;
    if (idx >= (long)A.C * L * Nu) return;
    const int j = (int)(idx % Nu);
    const long t = idx / Nu;
    const int i = (int)(t % L), c = (int)(t / L);
    const size_t qs = (size_t)L * Nu;                                      // doubles between the rows vp, vs, rho, h of jac
    double *jac = A.jac + ((size_t)c * 4 * L + i) * Nu + j;
    double *lay = (A.layer && j == 0) ? A.layer + (size_t)c * 4 * L + i : nullptr;
    if (layers_has_thermal(A.idesc) || i >= A.idesc[2]) {                  // a thermal layer: NaN for the whole chain, no scratch read
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        jac[0] = nan; jac[qs] = nan; jac[2 * qs] = nan; jac[3 * qs] = nan;
        if (lay) { lay[0] = nan; lay[L] = nan; lay[2 * L] = nan; lay[3 * L] = nan; }
        return;
    }
    const LayerDual o = layer_value_dual(A.idesc, A.fdesc, A.params + (size_t)c * A.N, i, j);
    jac[0] = o.d[0]; jac[qs] = o.d[1]; jac[2 * qs] = o.d[2]; jac[3 * qs] = o.d[3];
    if (lay) { lay[0] = o.v[0]; lay[L] = o.v[1]; lay[2 * L] = o.v[2]; lay[3 * L] = o.v[3]; }
}

hipError_t launch_params_jacobian(hipStream_t s, const ParamsJacArgs &a)
{
    const long total = (long)a.C * a.L * a.Nu;
    const long grid = (total + 255) / 256;
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(surfdisp_params_jacobian_kernel, dim3((unsigned)grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

__device__ __forceinline__ int plsq_tri(int i, int j) { return i * (i + 1) / 2 + j; }      // j <= i
__device__ __forceinline__ bool plsq_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

__global__ __launch_bounds__(256) void surfdisp_lsq_step_params_kernel(ParamLsqArgs A)
{
    constexpr int R = SD_LSQ_TILE_ROWS, NM = SD_PLSQ_MAX_UNKNOWNS, NF = NM + 1, CH = SD_PLSQ_CHUNK;
    __shared__ double M[NF * (NF + 1) / 2];          // packed lower triangle of the (n + 1) x (n + 1) augmented matrix
    __shared__ double Gt[R * NF];                    // [R][n + 1]: staged rows, column n = residual
    __shared__ float Pt[R * 4 * CH];                 // [R][K_b, K_a, K_rho, K_h][CH]: a chunk of the rows' kernels
    __shared__ double cv[256], dg[NF], dl[NF];
    __shared__ double sdiag[NF], sbeta[NF], sdp[NF]; // lam / scale^2 + beta, beta, p - ref of the free unknowns
    __shared__ int fidx[NF], pos[NM];
    __shared__ const float *rk[4][R];                // the row's kernels at its (stack, period): d/dVs, d/dVp, d/drho, d/dh
    __shared__ double rwr[R], rsg[R], rt[R];
    __shared__ int rok[R], rbad[R];
    __shared__ int sh_n, sh_flag;

    const int s = blockIdx.x, tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int Lmax = A.Lmax, Nu = A.Nu;
    int nl = A.nlay ? A.nlay[s] : Lmax;
    nl = nl < 0 ? 0 : (nl > Lmax ? Lmax : nl);
    const size_t ob = A.obs_per_stack ? (size_t)s * A.N : 0;
    const double *jac = A.jac + (size_t)s * 4 * Lmax * Nu;
    const size_t qs = (size_t)Lmax * Nu;

    // ---- the free unknowns of this stack, in order: fidx[k] = unknown of column k, pos[unknown] = k or -1
    if (tid < 64) {
        const unsigned char *fm = A.free_mask ? A.free_mask + (A.free_per_stack ? (size_t)s * Nu : 0) : nullptr;
        const bool f = tid < Nu && (!fm || fm[tid] != 0);
        const unsigned long long m = __ballot(f);
        const int k = __popcll(m & ((1ull << tid) - 1ull));
        if (f) fidx[k] = tid;
        if (tid < Nu) pos[tid] = f ? k : -1;
        if (tid == 0) { sh_n = __popcll(m); sh_flag = 0; }
    }
    __syncthreads();
    const int n = sh_n, n1 = n + 1;
    const int tot = n1 * (n1 + 1) / 2;
    const double lam = A.lam[s];
    for (int k = tid; k < n; k += 256) {
        const int u = fidx[k];
        const double sc = A.scale[u], beta = A.prior_w ? A.prior_w[u] : 0.0;
        sbeta[k] = beta;
        sdiag[k] = lam / (sc * sc) + beta;
        sdp[k] = A.prior_w ? A.params[(size_t)s * A.Np + u] - A.prior_ref[u] : 0.0;
    }
    for (int t = tid; t < tot; t += 256) M[t] = 0.0;
    __syncthreads();

    // Stage the rows r0 .. r0 + R - 1 into Gt: validity, weight, sign (the row rules of section (6d), and of (6h) for part_h), the
    // chain rule through jac, the drop of a row with a column that is not finite.  Called by the whole workgroup; ends on a barrier.
    auto stage = [&](int r0) {
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
                        kh = A.part_h[k];
                    }
                const int P = (sa >= 0 && sa <= 4) ? (sa >= 2 && sa <= 3 ? A.nper[1] : A.nper[0]) : 0;
                const double o = A.obs[ob + r], sgm = A.uncer[ob + r];
                const bool in = A.mask[ob + r] != 0 && plsq_finite(o) && plsq_finite(sgm) && sgm > 0.0;
                if (pp && in && idx >= 0 && idx < P) {
                    double v = (double)pp[(size_t)s * pst + idx];
                    bool solved;
                    if (sa == 4) {                                          // chi: finite, at a period whose root was found
                        solved = plsq_finite(v) && (double)A.pred[0][(size_t)s * A.pstride[0] + idx] >= 0.01;
                        if (src == 5 && v < 0.0) { sg = -1.0; v = -v; }     // |chi|: the row takes the sign of chi
                    } else
                        solved = v >= 0.01;
                    solved = solved && kh != nullptr;                       // the row names a missing thickness array
                    if (solved) {
                        ok = 1;
                        wr = A.weights[r] / (sgm * sgm);
                        res = o - v;
                        const size_t off = ((size_t)s * P + idx) * Lmax;
                        kb = kb ? kb + off : nullptr; ka = ka ? ka + off : nullptr; kr = kr ? kr + off : nullptr;
                        kh += off;
                    }
                }
            }
            rok[tid] = ok; rbad[tid] = 0; rwr[tid] = wr; rsg[tid] = sg;
            rk[0][tid] = kb; rk[1][tid] = ka; rk[2][tid] = kr; rk[3][tid] = kh;
            Gt[tid * n1 + n] = res;
        }
        for (int t = tid; t < R * n; t += 256) { const int rr = t / n; Gt[rr * n1 + (t - rr * n)] = 0.0; }
        __syncthreads();
        for (int c0 = 0; c0 < nl; c0 += CH) {
            for (int t = tid; t < R * 4 * CH; t += 256) {                  // consecutive lanes: consecutive layers of one kernel row
                const int rr = t / (4 * CH), q = (t / CH) & 3, i = c0 + (t & (CH - 1));
                const float *k = rk[q][rr];
                Pt[t] = (rok[rr] && k && i < (q == 3 ? nl - 1 : nl)) ? k[i] : 0.0f;
            }
            __syncthreads();
            const int ni = nl - c0 < CH ? nl - c0 : CH;
            for (int t = tid; t < R * n; t += 256) {                        // consecutive lanes: consecutive unknowns of one jac row
                const int rr = t / n, k = t - rr * n;
                if (rok[rr]) {
                    const double *jc = jac + (size_t)c0 * Nu + fidx[k];
                    const float *pr = Pt + rr * 4 * CH;
                    const bool hb = rk[0][rr] != nullptr, ha = rk[1][rr] != nullptr, hr = rk[2][rr] != nullptr;
                    double g = Gt[rr * n1 + k];
                    // selects, not branches: a skipped term adds an exact 0.0, and the loads of the next layers are not held back
#pragma unroll 4
                    for (int ii = 0; ii < ni; ++ii) {
                        const double jb = jc[qs + (size_t)ii * Nu], ja = jc[(size_t)ii * Nu], jr = jc[2 * qs + (size_t)ii * Nu];
                        const double jh = jc[3 * qs + (size_t)ii * Nu];    // (layer c0 + ii < nl <= Lmax: inside jac)
                        g += (hb && jb != 0.0) ? (double)pr[ii] * jb : 0.0;
                        g += (ha && ja != 0.0) ? (double)pr[CH + ii] * ja : 0.0;
                        g += (hr && jr != 0.0) ? (double)pr[2 * CH + ii] * jr : 0.0;
                        g += (c0 + ii < nl - 1 && jh != 0.0) ? (double)pr[3 * CH + ii] * jh : 0.0;
                    }
                    Gt[rr * n1 + k] = g;
                }
            }
            __syncthreads();
        }
        for (int t = tid; t < R * n; t += 256) {
            const int rr = t / n, k = t - rr * n;
            if (rok[rr]) {
                const double g = Gt[rr * n1 + k] * rsg[rr];
                if (!plsq_finite(g)) rbad[rr] = 1;                          // a NaN row of a failed unit: dropped
                Gt[rr * n1 + k] = g;
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
    int used = 0;                                                          // (the same count in every lane)
    for (int r0 = 0; r0 < A.N; r0 += R) {
        stage(r0);
        for (int i = ty; i <= n; i += 16)
            for (int j = tx; j <= i; j += 16) {
                double sum = 0.0;
                for (int rr = 0; rr < R; ++rr)
                    if (rok[rr]) sum += (rwr[rr] * Gt[rr * n1 + i]) * Gt[rr * n1 + j];
                M[plsq_tri(i, j)] += sum;
            }
        for (int rr = 0; rr < R; ++rr) used += rok[rr];
        __syncthreads();
    }

    // ---- damping and prior: lam / scale^2 + beta on the diagonal, -beta (p - ref) on row n; misfit and prior term at p
    double misfit = 0.0, prior = 0.0;                                      // (thread 0's copies count)
    if (tid == 0) {
        misfit = M[plsq_tri(n, n)];
        for (int k = 0; k < n; ++k) prior += sbeta[k] * sdp[k] * sdp[k];
        sh_flag = used == 0 ? 1 : 0;
    }
    for (int k = tid; k < n; k += 256) {
        M[plsq_tri(k, k)] += sdiag[k];
        M[plsq_tri(n, k)] -= sbeta[k] * sdp[k];
    }
    __syncthreads();
    int flag = sh_flag;

    // ---- Cholesky factorisation of the columns 0..n-1 over the rows 0..n (row n becomes y = L^-1 g), then L^T delta = y
    double logdet = 0.0;                                                   // (the same sum in every lane)
    if (flag == 0) {
        for (int k = 0; k < n; ++k) {
            const double d = M[plsq_tri(k, k)];                            // the same value in every lane: a uniform exit
            if (!(d > 0.0) || !plsq_finite(d)) { flag = 2; break; }
            const double l = sqrt(d);
            logdet += log(d);
            for (int i = k + tid; i <= n; i += 256) {
                if (i == k) dg[k] = l;
                else { const double v = M[plsq_tri(i, k)] / l; M[plsq_tri(i, k)] = v; cv[i] = v; }
            }
            __syncthreads();
            for (int i = k + 1 + ty; i <= n; i += 16) {
                const double ci = cv[i];
                for (int j = k + 1 + tx; j <= i; j += 16) M[plsq_tri(i, j)] -= ci * cv[j];
            }
            __syncthreads();
        }
    }
    if (flag == 0) {
        for (int j = tid; j < n; j += 256) cv[j] = M[plsq_tri(n, j)];
        __syncthreads();
        for (int k = n - 1; k >= 0; --k) {
            const double dk = cv[k] / dg[k];
            if (tid < k) cv[tid] -= M[plsq_tri(k, tid)] * dk;
            if (tid == k) { dl[k] = dk; if (!plsq_finite(dk)) sh_flag = 2; }
            __syncthreads();
        }
        flag = sh_flag;                                                    // (a step that overflowed counts as a failed pivot)
    }

    // ---- the objective the linear model predicts at p + delta: sum W (res - G delta)^2 + sum beta (p + delta - ref)^2
    double pred = misfit + prior;
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
        if (tid == 0)
            for (int k = 0; k < n; ++k) { const double y = sdp[k] + dl[k]; pred += sbeta[k] * y * y; }
    }

    // ---- cov = A^-1 in the triangle (rows 0..n-1): T = L^-1 in place, column by column from the right, then C = T^T T in place
    const bool want_cov = (A.cov || A.sigma) && flag == 0 && n > 0;
    if (want_cov) {
        __syncthreads();
        for (int i = tid; i < n; i += 256) { const double t = 1.0 / dg[i]; M[plsq_tri(i, i)] = t; sdiag[i] = t; }   // (sdiag is free by now)
        __syncthreads();
        if (tid == 0 && n >= 2) cv[((n - 2) & 1) * NM + n - 1] = M[plsq_tri(n - 1, n - 2)];
        __syncthreads();
        for (int j = n - 2; j >= 0; --j) {
            const double *c = cv + (j & 1) * NM;                           // c[k] = L_kj, k > j
            const double tjj = sdiag[j];
            for (int i = j + 1 + ty; i < n; i += 16) {
                const double *row = M + plsq_tri(i, 0);
                double sum = 0.0;
                for (int k = j + 1 + tx; k <= i; k += 16) sum += row[k] * c[k];
                sum += __shfl_xor(sum, 8, 16); sum += __shfl_xor(sum, 4, 16); sum += __shfl_xor(sum, 2, 16); sum += __shfl_xor(sum, 1, 16);
                if (tx == 0) M[plsq_tri(i, j)] = -sum * tjj;
            }
            if (j > 0)                                                     // the next column of L, untouched so far
                for (int i = j + tid; i < n; i += 256) cv[((j - 1) & 1) * NM + i] = M[plsq_tri(i, j - 1)];
            __syncthreads();
        }
        const int W = n <= 16 ? 16 : (n <= 32 ? 32 : 64), RB = 256 / W;
        const int a = tid / W, j = tid - a * W;
        for (int i0 = 0; i0 < n; i0 += RB) {
            for (int t = tid; t < RB * W; t += 256) {                      // cv[a][k] = T_{k, i0+a}, k >= i0 + a
                const int aa = t / W, k = t - aa * W, i = i0 + aa;
                if (i < n && k >= i && k < n) cv[aa * W + k] = M[plsq_tri(k, i)];
            }
            __syncthreads();
            const int i = i0 + a;
            double sum = 0.0;
            if (i < n && j <= i)
                for (int k = i; k < n; ++k) sum += cv[a * W + k] * M[plsq_tri(k, j)];
            __syncthreads();
            if (i < n && j <= i) M[plsq_tri(i, j)] = sum;
        }
        __syncthreads();
        for (int t = tid; t < n * (n + 1) / 2; t += 256)
            if (!plsq_finite(M[t])) sh_flag = 2;                           // an inverse that overflowed counts as a failed pivot
        __syncthreads();
        flag = sh_flag;
    }

    // ---- outputs: zeros for a flag, zeros at fixed unknowns
    if (tid < Nu) {
        const int k = pos[tid];
        A.delta[(size_t)s * Nu + tid] = (flag == 0 && k >= 0) ? dl[k] : 0.0;
        if (A.sigma) A.sigma[(size_t)s * Nu + tid] = (flag == 0 && k >= 0) ? sqrt(M[plsq_tri(k, k)]) : 0.0;
    }
    if (A.cov) {
        double *cov = A.cov + (size_t)s * Nu * Nu;
        for (int t = tid; t < Nu * Nu; t += 256) {
            const int a = t / Nu, b = t - a * Nu;
            const int ka = pos[a], kb = pos[b];
            cov[t] = (flag == 0 && ka >= 0 && kb >= 0) ? (ka >= kb ? M[plsq_tri(ka, kb)] : M[plsq_tri(kb, ka)]) : 0.0;
        }
    }
    if (tid == 0) {
        if (flag == 2) pred = misfit + prior;                              // (a flag raised by the inverse: the objective at p)
        A.stats[3 * (size_t)s] = misfit; A.stats[3 * (size_t)s + 1] = prior; A.stats[3 * (size_t)s + 2] = pred;
        A.info[3 * (size_t)s] = used; A.info[3 * (size_t)s + 1] = A.N - used; A.info[3 * (size_t)s + 2] = flag;
        if (A.logdet) A.logdet[s] = flag == 0 ? logdet : 0.0;
    }
}

hipError_t launch_lsq_step_params(hipStream_t s, const ParamLsqArgs &a)
{
    hipLaunchKernelGGL(surfdisp_lsq_step_params_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
