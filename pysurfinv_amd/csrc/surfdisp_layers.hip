// surfdisp_layers.hip -- parameters -> layer stack on the device, native counterpart
// of Model1D.seisPropLayers (models.py:72-102) + the layer classes of layers.py:139-284 for a model
// whose layer STRUCTURE is static (no thickness can cross a fine-layer threshold inside the prior
// box; decided on the host by Model1DBatch).  One thread per (chain, output layer).
//
// The host flattens the reference's `setting` into a descriptor:
//   idesc: [0]=nlayers_in  [1]=ngrid  [2]=L(out)  [3]=has_ref  then per input layer (8 ints):
//          kind, hslot, bottomdepth_flag, ncoef, grid_begin, grid_end, (first layer: slot + 1 of a per-row Info.topo,
//          0 = the constant z_start), 0 ; then coef slots
//          (nlayers_in x 8) ; then per output layer its top grid index (L ints)
//   fdesc: [0]=z_start ; per input layer (1+8 doubles): hconst, coefconst[8] ;
//          then per grid point (1+8 doubles): t in [0,1], basis row (vs = sum basis[k]*coef[k])
// kinds: 0 sed, 1 crust, 2 mantle, 3 water, 4 osed, 5 ocrust  (rules: layers.py, cited below),
//        6 thermal mantle (OceanMantleHybrid): vs, qs per grid point come from the scratch array
//        written by surfdisp_thermal_kernel (surfdisp_thermal.hip), 7 OceanSedimentCascadia
#include <hip/hip_runtime.h>
#include "surfdisp_internal.h"
#include "surfdisp_layers_grid.h"

namespace sd {

// (GridVal, closed_forms and grid_value, the seismic properties of one grid point: surfdisp_layers_grid.h, shared with
// surfdisp_mcmc_prior.hip)

__global__ __launch_bounds__(256) void surfdisp_layers_kernel(LayersArgs A)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int L = A.idesc[2];
    if (idx >= (long)A.C * L) return;
    const int c = (int)(idx / L), i = (int)(idx % L);
    const int nin = A.idesc[0];
    const int *top_i = A.idesc + 4 + 16 * nin;          // L ints behind the 8 + 8 ints per input layer
    const int g = top_i[i];
    const GridVal a = grid_value(A, c, g), b = grid_value(A, c, g + 1);
    float *m = A.model + (size_t)c * 5 * L;            // rows vp, vs, rho, h, 1/Qs (fast_surf.f:2-5)
    const double qs = (a.qs + b.qs) / 2;
    m[0 * L + i] = (float)((a.vp + b.vp) / 2);
    m[1 * L + i] = (float)((a.vs + b.vs) / 2);
    m[2 * L + i] = (float)((a.rho + b.rho) / 2);
    m[3 * L + i] = (float)(b.z - a.z);
    m[4 * L + i] = (float)(qs > 0 ? 1.0 / qs : 0.0);
}

// The GENERIC prior predicates of the reference's model classes (models.py:294-320 and alike: what every `isgood` there is
// built from) on the grid points of Model1D.seisPropGrids, one thread per (chain, output layer) - so that a sampler with a
// prior keeps its lock step on the device (MetropolisBatch, pysurfinv_amd.mcmc.PriorRules):
//   flags[i] bit 0: Vs must INCREASE across output layer i (bottom point - top point >= eps: monoIncrease, models.py:8-9,
//                   over the grid points of a group);
//            bit 1: ... and from its bottom point to the top point of output layer i + 1 (two input layers of one such group);
//            bit 2: Vs must not DROP from its bottom point to the top point of output layer i + 1 ("Vs jump between group is
//                   positive", models.py:302-307);
//            bit 3: the cap applies to its two points: Vs <= vs_max (models.py:309-313; not the ReferenceMantle's layers).
// tags [C]: a chain whose model breaks a rule gets tags[c] = mark_tag; only_tag >= 0: only the chains with tags[c] == only_tag are
// looked at (the ones the last masked redraw touched) - rounds of a step use rising tags, so nothing is cleared in between.
__global__ __launch_bounds__(256) void surfdisp_prior_kernel(LayersArgs A, const int *flags, double vs_max, int only_tag, int mark_tag,
                                                             unsigned char *tags)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int L = A.idesc[2];
    if (idx >= (long)A.C * L) return;
    const int c = (int)(idx / L), i = (int)(idx % L);
    // (a chain found bad by another of its threads already carries mark_tag > only_tag: still looked at, the outcome is the same)
    if (only_tag >= 0 && tags[c] < (unsigned char)only_tag) return;
    const int f = flags[i];
    if (f == 0) return;
    const int nin = A.idesc[0];
    const int *top_i = A.idesc + 4 + 16 * nin;
    const int g = top_i[i];
    const GridVal a = grid_value(A, c, g), b = grid_value(A, c, g + 1);
    const double eps = 2.220446049250313e-16;              // np.finfo(float).eps, models.py:8
    bool ok = true;
    if (f & 8) ok = ok && !(a.vs > vs_max) && !(b.vs > vs_max);
    if (f & 1) ok = ok && (b.vs - a.vs >= eps);
    if ((f & 6) && i + 1 < L) {
        const GridVal n = grid_value(A, c, top_i[i + 1]);
        if (f & 2) ok = ok && (n.vs - b.vs >= eps);
        if (f & 4) ok = ok && !(n.vs < b.vs);
    }
    if (!ok) tags[c] = (unsigned char)mark_tag;
}

hipError_t launch_prior(hipStream_t s, const LayersArgs &a, int L, const int *flags, double vs_max, int only_tag, int mark_tag,
                        unsigned char *tags)
{
    const long total = (long)a.C * L;
    const int grid = (int)((total + 255) / 256);
    hipLaunchKernelGGL(surfdisp_prior_kernel, dim3(grid), dim3(256), 0, s, a, flags, vs_max, only_tag, mark_tag, tags);
    return hipGetLastError();
}

hipError_t launch_layers(hipStream_t s, const LayersArgs &a, int L)
{
    const long total = (long)a.C * L;
    const int grid = (int)((total + 255) / 256);
    hipLaunchKernelGGL(surfdisp_layers_kernel, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
