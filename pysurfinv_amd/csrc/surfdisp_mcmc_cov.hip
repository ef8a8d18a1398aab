// surfdisp_mcmc_cov.hip -- proposals shaped by a covariance: x + F z with a per-point lower-triangular factor F, for every node of the
// speculative tree, redrawn INSIDE the kernel while the box or the prior's rules refuse the candidate
// (surfdisp_mcmc_propose_cov_device), and the factor itself, a Cholesky of scale^2 cov per point (surfdisp_mcmc_cov_factor_device);
// include/surfdisp.h section (6c).  A translation unit of its own: the propose, accept, stack and prior kernels of surfdisp_mcmc.hip
// and surfdisp_layers.hip keep their instruction streams (profiles/cov_proposal/isa_identity.txt); the random streams, the grid
// points and the test of a candidate row are shared (surfdisp_mcmc_rng.h, surfdisp_layers_grid.h, surfdisp_mcmc_rules.h).
//
// The reference's perturb redraws the WHOLE proposal while it is refused (models.py:192-205); so does this kernel, for the box too.
// Redrawing into a box makes the proposal density slightly asymmetric near the walls (the mass a wall cuts off is spread over the
// inside, and how much is cut off depends on where the chain stands) - exactly as the reference's per-scalar redraw does
// (brownian.py:20-27).  The sampler follows the reference there and does not correct for it: no Hastings term.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "surfdisp_internal.h"
#include "surfdisp_mcmc_rng.h"
#include "surfdisp_layers_grid.h"
#include "surfdisp_mcmc_rules.h"

namespace sd {

// One workgroup = one wavefront = one chain, lane n = scalar n (N <= 64): the retry loop's barriers are uniform by construction.
// Per node k of the tree (0, 1, ..., 2^depth - 2; node 0 draws from the chain's state, child 2k+1 from the final proposal of k, child
// 2k+2 from the state of k) and whole-proposal retry r = 0 .. gauss_tries + uniform_tries - 1:
//   r < gauss_tries: lane n draws z_n = sqrt(-2 log u1) cospi(2 u2) from ONE Philox call - word 1 the tag of Gaussian try 0 of node k,
//   stream index gidx + (r << 48), gidx = (chain0 + c) N + n: the counter words of surfdisp_mcmc_propose_kernel's first candidate with
//   the retry where surfdisp_mcmc_propose_prior_kernel puts it - and leaves it in LDS; after a barrier
//   cand_n = x_n + sum_{k <= n} L[n][k] z_k, k ascending, L the factor of the chain's point read from global memory as
//   factor_t[f][k][n] (the lanes read a column's entries side by side; the chains of a point share the factor, so it stays in L2);
//   r >= gauss_tries: draw_bounded's uniform branch on the same index - bit for bit the uniform phase of the prior kernel;
//   the candidate is good when every scalar lies strictly inside (vmin_n, vmax_n) (a wave vote) and, with flags, the prior's rules
//   hold on it (prior_rules_hold: the row and the Vs of its grid points in LDS); the first good candidate ends the loop.
// No good candidate within the caps: the node proposes the state it drew from, tries = the cap, *exhausted counts it.
// Node states are read from `p` or read back from `out` (every lane reads the element it wrote itself) at every retry: no private
// array indexed at run time (see the note in surfdisp_mcmc_propose_kernel), no scratch.  LDS: z [N], the row [N + K], the Vs of the
// grid points [L + SD_MCMC_PRIOR_GRID_EXTRA].  flags == nullptr: the box alone, no descriptor is touched (K = L = 0).
__global__ __launch_bounds__(64) void surfdisp_mcmc_propose_cov_kernel(McmcCovArgs A)
{
    extern __shared__ double lds[];                    // launch_mcmc_propose_cov sizes it: 2 N + K + L + SD_MCMC_PRIOR_GRID_EXTRA doubles
    const int lane = threadIdx.x;
    const size_t c = blockIdx.x;
    const int N = A.N, M = (1 << A.depth) - 1;
    double *zs = lds;                                  // the standard normals of one retry
    double *row = lds + N;                             // the candidate: [N random-walk scalars | K local constants]
    double *vsg = lds + 2 * N + A.K;                   // Vs of the candidate at every grid point the rules look at
    const int cap = A.gauss_tries + A.uniform_tries;
    const uint32_t k0 = (uint32_t)A.seed, k1 = (uint32_t)(A.seed >> 32);
    const long chain = A.chain0 + (long)c;
    const long gidx = chain * N + lane;                // (chain, parameter) of the whole sampler: the random stream's index
    const double *Lt = A.factor_t + (size_t)(chain / A.chains_per_factor) * N * N;
    const bool mine = lane < N;
    const double lo = mine ? A.vmin[lane] : 0.0, hi = mine ? A.vmax[lane] : 0.0;
    const bool ruled = A.flags != nullptr;
    const LayersArgs G{A.C, N + A.K, nullptr, A.idesc, A.fdesc, nullptr, nullptr};
    const int *top_i = nullptr;
    int L = 0, npts = 0;
    bool blocked = false;
    if (ruled) {
        prior_rule_setup(A.idesc, A.flags, A.L, lane, top_i, L, npts, blocked);
        for (int k = lane; k < A.K; k += 64) row[N + k] = A.aux[c * A.K + k];
    }
    const int ntry = blocked ? 0 : cap;
    const bool capped = !(A.vs_max < 0.0);
    for (int k = 0; k < M; ++k) {
        int j = k;                                     // the state of node k: the proposal of the last "accepted" edge above it
        for (int s = 0; s < SD_MCMC_MAX_DEPTH && j > 0 && !(j & 1); ++s) j = (j - 2) >> 1;
        const double *src = (j == 0) ? A.p + c * N : A.out + (c * M + ((j - 1) >> 1)) * N;
        const uint32_t w1 = (uint32_t)(A.counter >> 32) ^ ((uint32_t)k << 20);    // Gaussian try 0 of node k
        int found = cap;
        double cand = 0.0;
        for (int r = 0; r < ntry; ++r) {
            const long idx = gidx + ((long)r << 48);
            if (r < A.gauss_tries) {
                if (mine) {
                    const U4 q = philox4x32_10(U4{(uint32_t)A.counter, w1, (uint32_t)idx, (uint32_t)(idx >> 32)}, k0, k1);
                    zs[lane] = sqrt(-2.0 * log(u53(q.x, q.y))) * cospi(2.0 * u53(q.z, q.w));
                }
                __syncthreads();
                if (mine) {
                    double acc = 0.0;
                    for (int i = 0; i <= lane; ++i) acc += Lt[(size_t)i * N + lane] * zs[i];
                    cand = src[lane] + acc;
                }
            } else if (mine) {
                cand = draw_bounded(src[lane], lo, hi, 0.0, k0, k1, A.counter, (uint32_t)k, idx, true);
            }
            if (mine) row[lane] = cand;
            bool good = __all(!mine || (cand < hi && cand > lo)) != 0;          // the same on every lane
            if (good && ruled) {
                __syncthreads();
                good = prior_rules_hold(G, A.flags, A.vs_max, capped, top_i, L, npts, row, vsg, lane);
            }
            if (good) { found = r; break; }
            __syncthreads();                           // the next candidate overwrites z and the row
        }
        if (mine) A.out[(c * M + k) * N + lane] = (found < cap) ? cand : src[lane];
        if (lane == 0) {
            if (A.tries) A.tries[c * M + k] = (unsigned short)found;
            if (found == cap) atomicAdd(A.exhausted, 1);
        }
        __syncthreads();
    }
}

hipError_t launch_mcmc_propose_cov(hipStream_t s, const McmcCovArgs &a)
{
    // z, the row and the grid points' Vs: under 1.3 KB for the shipped models (a chain group's small kernels run beside the other
    // group's root search, which leaves 7 KB of a CU's LDS at full occupancy)
    const size_t bytes = (2 * (size_t)a.N + a.K + a.L + SD_MCMC_PRIOR_GRID_EXTRA) * sizeof(double);
    hipLaunchKernelGGL(surfdisp_mcmc_propose_cov_kernel, dim3((unsigned)a.C), dim3(64), bytes, s, a);
    return hipGetLastError();
}

// The factor of scale^2 cov [P][N][N] per point, in the propose kernel's layout factor_t[p][k][n] = L[n][k].  One wavefront per point,
// lane n = row n of L; the matrix sits in LDS as T[k][n] = A[n][k] (N N doubles: 32 KB at N = 64), so that the lanes' accesses to one
// column of L are side by side.  Right-looking Cholesky over the rows whose diagonal is not zero (a fixed parameter - zero row and
// column in cov - gets a zero row and column in L and never moves): per column j, the pivot d = T[j][j] must be positive and finite,
// l_n = T[j][n] / sqrt(d) for n > j, then T[k][n] -= l_n l_k for j < k <= n.  A bad pivot: flag[p] = 1 and the point gets
// diag(fallback_step), the reference's step - never a half-factored matrix (the output is written only after the last column).
__global__ __launch_bounds__(64) void surfdisp_mcmc_cov_factor_kernel(McmcCovFactorArgs A)
{
    extern __shared__ double T[];                      // [N][N]
    const int lane = threadIdx.x;
    const size_t pt = blockIdx.x;
    const int N = A.N;
    const double *cov = A.cov + pt * N * N;
    const double s2 = A.scale * A.scale;
    for (int e = lane; e < N * N; e += 64) T[e] = s2 * cov[e];          // symmetric: T[k][n] = A[n][k] = A[k][n]
    const bool mine = lane < N;
    const bool free_n = mine && cov[(size_t)lane * N + lane] != 0.0;
    const unsigned long long live = __ballot(free_n);  // the rows that take part: the same on every lane
    __syncthreads();
    bool bad = false;
    for (int j = 0; j < N && !bad; ++j) {
        if (!((live >> j) & 1)) continue;
        const double d = T[j * N + j];
        bad = !(d > 0.0 && isfinite(d));
        if (bad) break;
        const double s = sqrt(d);
        const bool below = free_n && lane > j;
        double l = 0.0;
        if (below) l = T[j * N + lane] / s;
        __syncthreads();                               // (every lane has read the pivot)
        if (below) T[j * N + lane] = l;
        if (lane == j) T[j * N + j] = s;
        __syncthreads();
        if (below)
            for (int k = j + 1; k <= lane; ++k)
                if ((live >> k) & 1) T[k * N + lane] -= l * T[j * N + k];
        __syncthreads();
    }
    double *out = A.factor_t + pt * N * N;
    for (int e = lane; e < N * N; e += 64) {
        const int k = e / N, n = e - k * N;
        double v = 0.0;
        if (bad) v = (k == n) ? A.fallback_step[n] : 0.0;
        else if (k <= n && ((live >> k) & 1) && ((live >> n) & 1)) v = T[e];
        out[e] = v;
    }
    if (lane == 0) A.flag[pt] = bad ? 1 : 0;
}

hipError_t launch_mcmc_cov_factor(hipStream_t s, const McmcCovFactorArgs &a)
{
    hipLaunchKernelGGL(surfdisp_mcmc_cov_factor_kernel, dim3((unsigned)a.P), dim3(64), (size_t)a.N * a.N * sizeof(double), s, a);
    return hipGetLastError();
}

}  // namespace sd
