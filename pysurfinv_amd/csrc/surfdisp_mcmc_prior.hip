// surfdisp_mcmc_prior.hip -- the proposal of a sampler with a prior, redrawn INSIDE the kernel until the prior's rules hold
// (surfdisp_mcmc_propose_prior_device, include/surfdisp.h section (6c)): what the reference's MCinv.perturb / reset do per
// chain (models.py:192-219: the whole proposal again, up to 1000 times with the bounded Gaussian step, then up to 10 000
// uniform prior draws), for every node of the speculative tree.  A translation unit of its own: the propose, accept, stack and
// prior kernels of surfdisp_mcmc.hip and surfdisp_layers.hip keep their instruction streams (profiles/prior_redraw/isa_identity.txt);
// the random streams and the grid points are theirs (surfdisp_mcmc_rng.h, surfdisp_layers_grid.h).  The test of a candidate row
// stands in surfdisp_mcmc_rules.h, shared with surfdisp_mcmc_cov.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "surfdisp_internal.h"
#include "surfdisp_mcmc_rng.h"
#include "surfdisp_layers_grid.h"
#include "surfdisp_mcmc_rules.h"

namespace sd {

// One workgroup = one wavefront = one chain, so the retry loop's barriers are uniform by construction and chains that need
// different numbers of tries never meet at one.  Per node k of the tree (0, 1, ..., 2^depth - 2; node 0 draws from the chain's
// state, child 2k+1 from the good proposal of k, child 2k+2 from the state of k) and retry r (r < gauss_tries: the bounded
// Gaussian step, then uniform_tries uniform draws):
//   the lanes stride over the N scalars and draw the candidate into the row in LDS - draw_bounded's own draws, stream index
//   gidx + (r << 48): r = 0 is the draw of surfdisp_mcmc_propose_kernel;
//   the lanes stride over the grid points and put the row's Vs there into LDS (grid_value reads the [N + K] row from LDS: the K
//   local constants are put there once), then over the L output layers with surfdisp_prior_kernel's statements on those values -
//   a grid point is evaluated once, not once per layer that looks at it: at 25 600 chains the kernel is bound by the divergent
//   loads of the descriptor inside grid_value;
//   a wave vote ends the loop at the first good candidate.
// No good candidate within the caps: the node proposes the state it drew from, tries = the cap, *exhausted counts it.
// Node states are read from `p` or read back from `out` (every lane reads the elements it wrote itself) at every retry: no private
// array indexed at run time (see the note in surfdisp_mcmc_propose_kernel), no scratch, and no LDS beyond the row and the Vs.
// A descriptor with a thermal layer (kind 6) has no scratch array here, one with more grid points than L output layers can have
// (L + SD_MCMC_PRIOR_GRID_EXTRA) no room: every node is reported exhausted, nothing is read.
__global__ __launch_bounds__(64) void surfdisp_mcmc_propose_prior_kernel(McmcPriorArgs A)
{
    extern __shared__ double lds[];                    // launch_mcmc_propose_prior sizes it: N + K + gcap doubles
    const int lane = threadIdx.x;
    const size_t c = blockIdx.x;
    const int N = A.N, M = (1 << A.depth) - 1;
    double *row = lds;                                 // the candidate: [N random-walk scalars | K local constants]
    double *vsg = lds + N + A.K;                       // Vs of the candidate at every grid point the rules look at: gcap doubles
    const int cap = A.gauss_tries + A.uniform_tries;
    const uint32_t k0 = (uint32_t)A.seed, k1 = (uint32_t)(A.seed >> 32);
    const long gidx0 = (A.chain0 + (long)c) * N;       // (chain, parameter 0) of the whole sampler: the random stream's index
    const LayersArgs G{A.C, N + A.K, nullptr, A.idesc, A.fdesc, nullptr, nullptr};
    const int *top_i;
    int L, npts;
    bool blocked;
    prior_rule_setup(A.idesc, A.flags, A.L, lane, top_i, L, npts, blocked);
    const int ntry = blocked ? 0 : cap;
    const bool capped = !(A.vs_max < 0.0);
    for (int k = lane; k < A.K; k += 64) row[N + k] = A.aux[c * A.K + k];
    for (int k = 0; k < M; ++k) {
        int j = k;                                     // the state of node k: the proposal of the last "accepted" edge above it
        for (int s = 0; s < SD_MCMC_MAX_DEPTH && j > 0 && !(j & 1); ++s) j = (j - 2) >> 1;
        const double *src = (j == 0) ? A.p + c * N : A.out + (c * M + ((j - 1) >> 1)) * N;
        int found = cap;
        for (int r = 0; r < ntry; ++r) {
            for (int n = lane; n < N; n += 64)
                row[n] = draw_bounded(src[n], A.vmin[n], A.vmax[n], A.step[n], k0, k1, A.counter, (uint32_t)k,
                                      gidx0 + n + ((long)r << 48), r >= A.gauss_tries);
            __syncthreads();
            const bool good = prior_rules_hold(G, A.flags, A.vs_max, capped, top_i, L, npts, row, vsg, lane);
            if (good) { found = r; break; }
            __syncthreads();                           // the next candidate overwrites the row
        }
        double *o = A.out + (c * M + k) * N;
        for (int n = lane; n < N; n += 64) o[n] = (found < cap) ? row[n] : src[n];
        if (lane == 0) {
            if (A.tries) A.tries[c * M + k] = (unsigned short)found;
            if (found == cap) atomicAdd(A.exhausted, 1);
        }
        __syncthreads();
    }
}

hipError_t launch_mcmc_propose_prior(hipStream_t s, const McmcPriorArgs &a)
{
    // the row and the grid points' Vs, nothing else: under a kilobyte for the shipped models (a root search at full occupancy
    // leaves 7 KB of a CU's LDS, and a chain group's small kernels run beside the other group's root search)
    const size_t bytes = ((size_t)a.N + a.K + a.L + SD_MCMC_PRIOR_GRID_EXTRA) * sizeof(double);
    hipLaunchKernelGGL(surfdisp_mcmc_propose_prior_kernel, dim3((unsigned)a.C), dim3(64), bytes, s, a);
    return hipGetLastError();
}

}  // namespace sd
