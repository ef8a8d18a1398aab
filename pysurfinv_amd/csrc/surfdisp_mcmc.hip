// surfdisp_mcmc.hip -- the Metropolis glue of one lock step on the device: what the reference does per
// step and chain in Python - BrownianVar.move for every random-walk scalar (brownian.py:20-27), Point.misfit
// (point.py:15-31) and the accept rule (point.py:34-37) - as two kernels around the forward solve, so that a lock step is
// propose -> parameters->stacks -> prep / root search / finish -> accept: six launches instead of ~45 torch kernels and
// two host synchronisations (25 600 chains x 96 layers: 0.38 ms of a 7.1 ms lock step).
// Random numbers: Philox4x32-10 (Salmon et al. 2011), keyed by the caller's seed, counter = (call counter, element,
// draw index): reproducible for a given (seed, counter), independent of the launch geometry.  Statistical parity with
// the reference's Mersenne Twister stream, like the torch generator it replaces (pysurfinv_amd.brownian).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "surfdisp_internal.h"
#include "surfdisp_mcmc_rng.h"

namespace sd {

// (Philox4x32-10, u53 and draw_bounded, the bounded Gaussian step: surfdisp_mcmc_rng.h, shared with surfdisp_mcmc_prior.hip)

// One thread per (chain, parameter).  depth <= 1: one proposal, out [C][N].  depth d > 1 (speculative sampler): the binary
// tree of the next d accept / reject outcomes - node k's proposal is drawn from the state its branch would be in (node 0:
// the chain's state; child 2k+1 "accepted": the proposal of k; child 2k+2 "rejected": the state of k), out [C][2^d - 1][N].
// Every scalar moves independently (brownian.py), so a thread builds the whole tree of its own parameter.
__global__ __launch_bounds__(256) void surfdisp_mcmc_propose_kernel(McmcProposeArgs A)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)A.C * A.N) return;
    const int n = (int)(idx % A.N);
    const long c = idx / A.N;
    const double lo = A.vmin[n], hi = A.vmax[n], s = A.step[n];
    const uint32_t k0 = (uint32_t)A.seed, k1 = (uint32_t)(A.seed >> 32);
    const long gidx = idx + A.chain0 * A.N;                             // (chain, parameter) of the whole sampler: the random stream's index
    if (A.redo) {
        // masked redraw (a sampler with prior rules, MetropolisBatch): only the chains whose last proposal broke a rule draw
        // again - try number A.attempt of this step (its own random numbers); reset 2: the chain's state itself (no proposal)
        if (A.redo[c] != (unsigned char)A.redo_tag) return;
        A.out[idx] = (A.reset == 2) ? A.p[idx]
                                    : draw_bounded(A.p[idx], lo, hi, s, k0, k1, A.counter, 64u + (uint32_t)A.attempt, gidx, A.reset != 0);
        return;
    }
    const int M = A.depth > 1 ? (1 << A.depth) - 1 : 1;
    double S[SD_MCMC_MAX_NODES];
    S[0] = A.p[idx];
    // fully unrolled: every index of S is a compile-time constant.  (With a run-time index the register array is written
    // through s_set_gpr_idx BEFORE the bounds test selects the result - hipcc 7.2 speculates the guarded stores - and the
    // out-of-range writes of the nodes 7..14 of a depth-4 tree land in the neighbouring live registers, the output pointer
    // among them: a memory fault, found on the first depth-4 run.)
#pragma unroll
    for (int k = 0; k < SD_MCMC_MAX_NODES; ++k) {
        if (k < M) {
            const double x = S[k];
            const double nv = draw_bounded(x, lo, hi, s, k0, k1, A.counter, (uint32_t)k, gidx, A.reset != 0);
            A.out[((size_t)c * M + k) * A.N + n] = nv;
            if (2 * k + 2 < SD_MCMC_MAX_NODES) { S[2 * k + 1] = nv; S[2 * k + 2] = x; }
        }
    }
}

// misfit of one predicted curve against a chain's observations: (misfit, chi-square with the reference's clamp, L)
__device__ __forceinline__ void misfit_of(const McmcAcceptArgs &A, const float *cp, bool failed, size_t ob,
                                          double &mis, double &chi, double &L)
{
    chi = 0.0;
    int cnt = 0;
    for (int k = 0; k < A.P; ++k) {
        const double v = (double)cp[k];
        if (v < 0.01) failed = true;                                   // models.py:29-33
        if (A.mask[ob + k]) {
            const double r = (A.c_obs[ob + k] - v) / A.uncer[ob + k];
            chi += r * r;
            ++cnt;
        }
    }
    mis = sqrt(chi / (double)cnt);                                     // point.py:27-31
    if (!(chi < 50.0)) chi = sqrt(chi * 50.0);
    L = exp(-0.5 * chi);
    if (failed) { mis = 88888.0; chi = 88888.0; L = 0.0; }             // point.py:20-21
}

// One chain's Metropolis test(s): misfit of the proposal against the chain's observations, accept rule, state update, mcTrack row.
// depth d > 1: the chain walks the tree of surfdisp_mcmc_propose_kernel for nsteps <= d steps - at node k the usual test of
// proposal k against the current state, then child 2k+1 (accepted) or 2k+2 - one mcTrack row per step, step_stride doubles
// apart.  Every proposal was drawn from the state the chain is in when it is tested, so the chain is the plain sampler's.
// misfit(q, ob, mis, chi, L): the misfit of stack q of the batched solve against the observations at offset ob.
template <class Misfit>
__device__ __forceinline__ void accept_walk(const McmcAcceptArgs &A, int c, Misfit misfit)
{
    const int N = A.N;
    const int M = A.depth > 1 ? (1 << A.depth) - 1 : 1;
    const int nsteps = A.depth > 1 ? A.nsteps : 1;
    const size_t ob = A.obs_per_chain ? (size_t)c * A.P : 0;
    const unsigned long long gc = (unsigned long long)(A.chain0 + c);
    double *p0 = A.p0 + (size_t)c * N;
    double chi0 = A.chi0[c];
    int node = 0;
    for (int s = 0; s < nsteps; ++s) {
        const size_t q = (size_t)c * M + node;                         // this step's proposal: stack q of the batched solve
        double mis, chi, L;
        misfit(q, ob, mis, chi, L);
        bool acc;
        if (A.first) acc = true;                                       // a chain's first row: the start model itself
        else if (chi < chi0) acc = true;                               // point.py:34-37
        else {
            const U4 r = philox4x32_10(U4{(uint32_t)A.counter, (uint32_t)(A.counter >> 32) ^ 0x00aaaa00u ^ ((uint32_t)s << 28),
                                          (uint32_t)gc, (uint32_t)(gc >> 32)}, (uint32_t)A.seed, (uint32_t)(A.seed >> 32));
            const double u = u53(r.x, r.y);
            acc = u > 1.0 - exp(-(chi - chi0) / 2.0);
        }
        const double *p1 = A.p1 + q * N;
        if (A.row) {
            double *row = A.row + (size_t)c * A.row_stride + (size_t)s * A.step_stride;
            row[0] = mis; row[1] = L; row[2] = acc ? 1.0 : 0.0;
            for (int n = 0; n < N; ++n) row[3 + n] = p1[n];
        }
        if (acc) {
            for (int n = 0; n < N; ++n) p0[n] = p1[n];
            chi0 = chi;
        }
        node = acc ? 2 * node + 1 : 2 * node + 2;
    }
    A.chi0[c] = chi0;
}

// One thread per chain: accept_walk with the Rayleigh phase-velocity misfit.
__global__ __launch_bounds__(256) void surfdisp_mcmc_accept_kernel(McmcAcceptArgs A)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= A.C) return;
    accept_walk(A, c, [&](size_t q, size_t ob, double &mis, double &chi, double &L) {
        misfit_of(A, A.c + q * A.P, A.status && A.status[q] != 0, ob, mis, chi, L);
    });
}

// Joint misfit of stack q (pysurfinv_amd/obsdata.py): chi2 = sum over the columns, in ascending order, of w ((obs - pred) / uncer)^2
// over the masked-in entries, N = their count.  Failed: a wave type with data whose status is not 0 or whose phase velocity is
// below 0.01 at any period of its solve, or a group velocity that a column reads that is not >= 0.01 (NaN included).  col[j]:
// the block's copy of the column table in LDS, source << 16 | period index, or -1 for a column that names a missing array or a
// period beyond its solve (it fails the model: no read out of bounds).  With one Rayleigh-phase data set of weight 1 this gives
// misfit_of's bits (the same operations on the masked-in entries, an exact +0 for the others).  The loops are unrolled so that
// one thread has several columns' loads in flight: at 100 chains the kernel is bound by the latency of those loads.
// E (surfdisp_mcmc_accept_joint5_device): a fifth prediction array, the Rayleigh ellipticity chi of the Rayleigh solve (pred[4],
// [stacks][nper[0]]), read by the sources 4 (chi as it is) and 5 (|chi|); a value a column reads that is not finite fails the
// model - no lower bound, chi <= 0 is a legitimate prediction.  The sources 0..3 go through the same operations in the same
// order with and without E (the kernels of the four-array entries are the E = false instantiation), and the source select stays
// a chain of compares on scalars: no indexed private array, no scratch.
template <bool E>
__device__ __forceinline__ void joint_misfit_of(const McmcJointArgs &J, const int *col, const double *wt, size_t q, size_t ob,
                                                double &mis, double &chi, double &L)
{
    const McmcAcceptArgs &A = J.a;
    bool failed = false;
    for (int w = 0; w < 2; ++w) {
        const float *cw = J.pred[2 * w];
        if (!cw) continue;
        if (J.status[w] && J.status[w][q] != 0) failed = true;
        cw += q * J.pstride[2 * w];
        float m = cw[0];                                               // (fminf skips NaN, as the test v < 0.01 does)
#pragma unroll 8
        for (int k = 1; k < J.nper[w]; ++k) m = fminf(m, cw[k]);
        if ((double)m < 0.01) failed = true;                           // models.py:29-33, per wave type
    }
    const float *base[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) base[k] = J.pred[k] ? J.pred[k] + q * J.pstride[k] : nullptr;
    const float *base4 = (E && J.pred[4]) ? J.pred[4] + q * J.pstride[4] : nullptr;
    chi = 0.0;
    int cnt = 0;
    // every load of a column is unconditional (a masked-out entry adds an exact 0), so the unrolled loop keeps them in flight
#pragma unroll 8
    for (int j = 0; j < A.P; ++j) {
        const int e = col[j];
        const bool in = A.mask[ob + j] != 0;
        const double o = A.c_obs[ob + j], sg = A.uncer[ob + j];
        if (e < 0) { failed = true; continue; }
        const int s = e >> 16;
        const float *b = s == 0 ? base[0] : s == 1 ? base[1] : s == 2 ? base[2] : (!E || s == 3) ? base[3] : base4;
        double v = (double)b[e & 0xffff];
        if (E && s >= 4) {
            if (!(fabs(v) <= 1.7976931348623157e308)) failed = true;   // an ellipticity the data use: NaN or inf
            if (s == 5) v = fabs(v);                                   // a measured H/V curve: |chi|
        } else if ((s & 1) && !(v >= 0.01)) failed = true;             // a group velocity the data use
        const double r = in ? (o - v) / sg : 0.0;
        chi += (wt[j] * r) * r;
        cnt += in ? 1 : 0;
    }
    mis = sqrt(chi / (double)cnt);
    if (!(chi < 50.0)) chi = sqrt(chi * 50.0);
    L = exp(-0.5 * chi);
    if (failed) { mis = 88888.0; chi = 88888.0; L = 0.0; }
}

// surfdisp_mcmc_accept_kernel with the joint misfit (accept_walk: the same accept rule, random stream, tree walk and mcTrack rows).
template <bool E>
__global__ __launch_bounds__(256) void surfdisp_mcmc_accept_joint_kernel(McmcJointArgs J)
{
    const McmcAcceptArgs &A = J.a;
    __shared__ int col[SD_MCMC_JOINT_MAX_COLS];
    __shared__ double wt[SD_MCMC_JOINT_MAX_COLS];
    for (int j = threadIdx.x; j < A.P; j += blockDim.x) {
        const int s = J.cols[2 * j], i = J.cols[2 * j + 1];
        // (sources 4 and 5 both read pred[4], at a period of the Rayleigh solve)
        const bool ell = E && (s == 4 || s == 5);
        const bool ok = (ell ? J.pred[4] != nullptr : (s >= 0 && s <= 3 && J.pred[s])) && i >= 0 && i < J.nper[ell ? 0 : s >> 1];
        col[j] = ok ? (s << 16) | i : -1;
        wt[j] = J.weights[j];
    }
    __syncthreads();
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= A.C) return;
    accept_walk(A, c, [&](size_t q, size_t ob, double &mis, double &chi, double &L) {
        joint_misfit_of<E>(J, col, wt, q, ob, mis, chi, L);
    });
}

hipError_t launch_mcmc_accept_joint(hipStream_t s, const McmcJointArgs &a, bool ellip)
{
    const dim3 grid((unsigned)((a.a.C + 255) / 256));
    if (ellip) hipLaunchKernelGGL(surfdisp_mcmc_accept_joint_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(surfdisp_mcmc_accept_joint_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mcmc_propose(hipStream_t s, const McmcProposeArgs &a)
{
    const long total = (long)a.C * a.N;
    hipLaunchKernelGGL(surfdisp_mcmc_propose_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mcmc_accept(hipStream_t s, const McmcAcceptArgs &a)
{
    hipLaunchKernelGGL(surfdisp_mcmc_accept_kernel, dim3((unsigned)((a.C + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
