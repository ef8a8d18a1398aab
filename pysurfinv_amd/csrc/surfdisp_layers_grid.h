// surfdisp_layers_grid.h -- the grid points of the params -> stack descriptor (see surfdisp_layers.hip for its layout): the closed
// forms of the layer classes and grid_value, shared by surfdisp_layers.hip (the stack kernel, the prior kernel) and
// surfdisp_mcmc_prior.hip (the redraw loop of a sampler with a prior, which reads a candidate row held in LDS).  The functions
// stand here as they stood in surfdisp_layers.hip; grid_value takes the row of the chain as a pointer.
#pragma once
#include <hip/hip_runtime.h>
#include "surfdisp_internal.h"

namespace sd {

struct GridVal { double z, vs, vp, rho, qs; };

__device__ __forceinline__ void closed_forms(int kind, double vs, double &vp, double &rho, double &qs)
{
    switch (kind) {
        case 0:  // Sediment, layers.py:150-155
            vp = vs * 2.0;
            rho = 1.22679 + 1.53201 * vs - 0.83668 * vs * vs + 0.20673 * vs * vs * vs - 0.01656 * vs * vs * vs * vs;
            qs = 80.0; break;
        case 1:  // Crust, layers.py:179-184
            vp = vs * 1.80;
            rho = 1.22679 + 1.53201 * vs - 0.83668 * vs * vs + 0.20673 * vs * vs * vs - 0.01656 * vs * vs * vs * vs;
            qs = 600.0; break;
        case 2:  // OceanMantle / Mantle, layers.py:262-267
            vp = vs * 1.76; rho = 3.4268 + (vs - 4.5) / 4.5; qs = 150.0; break;
        case 3:  // OceanWater, layers.py:187-199
            vp = 1.475; rho = 1.027; qs = 10000.0; break;
        case 4:  // OceanSediment, layers.py:208-213
            vp = vs * 1.23 + 1.28; rho = 0.541 + 0.3601 * vp; qs = 80.0; break;
        case 6:  // OceanMantleHybrid._calOthers, layers.py:350-363: qs is set by the caller
            vp = vs * 1.76; rho = 3.4268 + (vs - 4.5) / 4.5; break;
        case 7:  // OceanSedimentCascadia = OceanSediment rules, layers.py:288-295
            vp = vs * 1.23 + 1.28; rho = 0.541 + 0.3601 * vp; qs = 80.0; break;
        default: // OceanCrust, layers.py:223-228
            vp = vs * 1.8; rho = 0.541 + 0.3601 * vp; qs = 350.0; break;
    }
}

// the seismic properties of grid point g of chain c (Model1D.seisPropGrids' points: every input layer's N + 1 points, then
// the 21 of the ReferenceMantle) - shared by the stack kernel and the prior kernel.  p: the chain's row [random-walk parameters |
// per-point local constants], in global memory or in LDS; c indexes the thermal layer's scratch alone.
__device__ __forceinline__ GridVal grid_value(const LayersArgs &A, const int c, const double *p, const int g)
{
    const int nin = A.idesc[0], ngrid = A.idesc[1];
    const int *lay_i = A.idesc + 4;                    // 8 ints per input layer
    const int *coef_i = lay_i + 8 * nin;               // 8 slots per input layer
    const double *lay_f = A.fdesc + 1;                 // 9 doubles per input layer
    const double *grid_f = lay_f + 9 * nin;            // 9 doubles per grid point

    // layer tops (a handful of layers): zbot[l] = z_start + sum of the thicknesses above
    // A row of `params` is [random-walk parameters | per-point local constants] (Model1DBatch.set_local_info): both are
    // read through slot indices.  Stack top z0 = -max(topo, 0), models.py:74.
    // No register-resident arrays indexed at run time (hipcc 7.2 lowers those to s_set_gpr_idx moves and speculates guarded
    // indexed stores: scripts/microbench/gpr_idx_guard.hip; tests/test_isa_guard.py): the top and thickness of ONE input layer
    // are re-derived by walking the handful of layers above it.
    const double z0 = (lay_i[6] > 0) ? -fmax(p[lay_i[6] - 1], 0.0) : A.fdesc[0];
    auto layer_span = [&](int lq, double &zt, double &Hq) -> double {   // returns the bottom of the last input layer
        double z = z0;
        zt = z0; Hq = 0.0;
        for (int l = 0; l < nin; ++l) {
            const int hs = lay_i[8 * l + 1];
            double H = (hs >= 0) ? p[hs] : lay_f[9 * l];
            if (lay_i[8 * l + 2]) H = H - z;           // BottomDepth, layers.py:119-124
            if (l == lq) { zt = z; Hq = H; }
            z += H;
        }
        return z;
    };
    GridVal v;
    if (g < ngrid) {
        int l = 0;
        while (l + 1 < nin && g >= lay_i[8 * l + 5]) ++l;
        const double *gf = grid_f + 9 * g;
        double zt, Hq;
        (void)layer_span(l, zt, Hq);
        v.z = zt + gf[0] * Hq;
        double vs = 0.0;
        const int kind = lay_i[8 * l];
        if (kind == 6) {
            const double *sc = A.scratch + ((size_t)c * 64 + (g - lay_i[8 * l + 4])) * 2;
            vs = sc[0]; v.qs = sc[1];
        } else if (kind == 7) {
            const double H = Hq;
            vs = (0.02 * (H * H) + 1.27 * H + 0.29 * 0.1) / (H + 0.29);
        } else {
            const int nc = lay_i[8 * l + 3];
            for (int k = 0; k < nc; ++k) {
                const int sl = coef_i[8 * l + k];
                vs += gf[1 + k] * ((sl >= 0) ? p[sl] : lay_f[9 * l + 1 + k]);
            }
        }
        v.vs = vs;
        closed_forms(kind, vs, v.vp, v.rho, v.qs);
    } else {
        // ReferenceMantle (layers.py:267-284): 21 points over 300 km hanging off the last grid point
        const int gl = ngrid - 1;
        int l = nin - 1;
        const double *gf = grid_f + 9 * gl;
        double zt, Hq;
        const double zref = layer_span(l, zt, Hq);    // top of the ReferenceMantle
        double vs0 = 0.0, vp0, rho0, qs0 = 0.0;
        if (lay_i[8 * l] == 6) {
            const double *sc = A.scratch + ((size_t)c * 64 + (gl - lay_i[8 * l + 4])) * 2;
            vs0 = sc[0]; qs0 = sc[1];
        } else if (lay_i[8 * l] == 7) {
            vs0 = (0.02 * (Hq * Hq) + 1.27 * Hq + 0.29 * 0.1) / (Hq + 0.29);
        } else {
            const int nc = lay_i[8 * l + 3];
            for (int k = 0; k < nc; ++k) {
                const int sl = coef_i[8 * l + k];
                vs0 += gf[1 + k] * ((sl >= 0) ? p[sl] : lay_f[9 * l + 1 + k]);
            }
        }
        closed_forms(lay_i[8 * l], vs0, vp0, rho0, qs0);
        const double t = (double)(g - ngrid) / 20.0;
        const double zr = t * 300.0;
        v.z = zref + zr;
        v.vs = vs0 + zr * (0.35 / 200);
        v.vp = vp0 + (v.vs * 1.76 - vs0 * 1.76);
        v.rho = rho0 + ((3.4268 + (v.vs - 4.5) / 4.5) - (3.4268 + (vs0 - 4.5) / 4.5));
        v.qs = qs0;
    }
    return v;
}
// ... of chain c's row of A.params (the kernels of surfdisp_layers.hip)
__device__ __forceinline__ GridVal grid_value(const LayersArgs &A, const int c, const int g)
{
    return grid_value(A, c, A.params + (size_t)c * A.N, g);
}

}  // namespace sd
