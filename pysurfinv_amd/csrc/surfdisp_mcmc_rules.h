// surfdisp_mcmc_rules.h -- the prior's rules on one candidate row held in LDS, for the propose kernels that redraw a whole proposal
// until the rules hold: surfdisp_mcmc_prior.hip (the reference's axis-aligned step) and surfdisp_mcmc_cov.hip (the step shaped by a
// covariance factor).  The statements are those that stood in surfdisp_mcmc_propose_prior_kernel (what the move did to its listing:
// profiles/cov_proposal/isa_identity.txt); they are surfdisp_prior_kernel's on the values of grid_value (surfdisp_layers_grid.h).
#pragma once
#include <hip/hip_runtime.h>
#include "surfdisp_internal.h"
#include "surfdisp_layers_grid.h"

namespace sd {

// What a chain's wavefront works out once (every lane calls it; Lout: the caller's output layers).  -> top_i: the top grid point of every output layer; L: the output layers; npts: the grid points the flagged layers read; blocked:
// a descriptor with a thermal layer (kind 6) has no scratch array here, one with more grid points than L output layers can have
// (L + SD_MCMC_PRIOR_GRID_EXTRA) no room - nothing may be read through it.
__device__ __forceinline__ void prior_rule_setup(const int *idesc, const int *flags, int Lout, int lane, const int *&top_i, int &L, int &npts,
                                                 bool &blocked)
{
    const int gcap = Lout + SD_MCMC_PRIOR_GRID_EXTRA;
    const int nin = idesc[0];
    top_i = idesc + 4 + 16 * nin;
    L = Lout < idesc[2] ? Lout : idesc[2];
    bool thermal = false;
    for (int l = 0; l < nin; ++l) thermal = thermal || idesc[4 + 8 * l] == 6;
    // grid points the flagged layers read: a layer's two points and the top of the next layer - the model's own ngrid points, and
    // the ReferenceMantle's 21 behind them only where a flag reaches that far (PriorRules never sets one there)
    const int ngrid = idesc[1];
    bool far = false;
    for (int i = lane; i < L; i += 64) {
        const int f = flags[i];
        if (f != 0) far = far || top_i[i] + 1 >= ngrid || ((f & 6) && i + 1 < L && top_i[i + 1] >= ngrid);
    }
    npts = __any(far) ? ngrid + 21 : ngrid;
    blocked = thermal || npts > gcap;
}

// The rules on the candidate `row` (in LDS, complete: the caller has synchronised after writing it; G: the descriptor's view with rows
// of N + K doubles): the lanes stride over the grid points and put the row's Vs there into vsg (LDS, npts doubles), then over the L
// output layers with surfdisp_prior_kernel's statements on those values - a grid point is evaluated once, not once per layer that
// looks at it.  The same answer on every lane.
__device__ __forceinline__ bool prior_rules_hold(const LayersArgs &G, const int *flags, double vs_max, bool capped, const int *top_i, int L,
                                                 int npts, const double *row, double *vsg, int lane)
{
    const double eps = 2.220446049250313e-16;          // np.finfo(float).eps, models.py:8
    // every grid point once (surfdisp_prior_kernel evaluates a layer's three points per thread: the same values)
    for (int g = lane; g < npts; g += 64) vsg[g] = grid_value(G, 0, row, g).vs;
    __syncthreads();
    bool ok = true;
    for (int i = lane; i < L; i += 64) {
        const int f = flags[i];
        if (f == 0) continue;
        const int g = top_i[i];
        const double a = vsg[g], b = vsg[g + 1];
        if ((f & 8) && capped) ok = ok && !(a > vs_max) && !(b > vs_max);
        if (f & 1) ok = ok && (b - a >= eps);
        if ((f & 6) && i + 1 < L) {
            const double n = vsg[top_i[i + 1]];
            if (f & 2) ok = ok && (n - b >= eps);
            if (f & 4) ok = ok && !(n < b);
        }
    }
    return __all(ok) != 0;                             // the same on every lane
}

}  // namespace sd
