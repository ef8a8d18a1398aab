// surfdisp_layers_dual.h -- the params -> stack map of surfdisp_layers_grid.h / surfdisp_layers.hip as DUAL NUMBERS for ONE
// unknown j: every quantity carries its value and its partial derivative with respect to parameter slot j of the chain's row
// (include/surfdisp.h section (6i); csrc/surfdisp_lsq_params.hip).  A separate statement, host- and device-callable
// (tests/hostcheck/jaccheck.hip runs it on the host), so that surfdisp_layers_grid.h and the kernels that include it keep their
// instruction streams.  The VALUE part repeats the expressions of grid_value / closed_forms / surfdisp_layers_kernel line by line -
// tests/test_param_jacobian_gpu.py pins float32(layer) to the stack kernel's model bit for bit.
// One scalar derivative beside each value: no array over the unknowns in registers (tests/test_isa_guard.py).
// The thermal layer (kind 6) has no derivative here: layers_has_thermal() tells the caller, who writes NaN and reads no scratch.
#pragma once
#include <hip/hip_runtime.h>

#ifndef SD_HD
#define SD_HD __host__ __device__
#endif

namespace sd {

struct GridDual { double z, vs, vp, rho, dz, dvs, dvp, drho; };
struct LayerDual { double v[4], d[4]; };     // vp, vs, rho, h of one output layer (the row order of `model`) and d/dp_j

SD_HD __forceinline__ bool layers_has_thermal(const int *idesc)
{
    const int nin = idesc[0];
    bool t = false;
    for (int l = 0; l < nin; ++l) t = t || idesc[4 + 8 * l] == 6;
    return t;
}

// closed_forms with the derivative: (vp, rho) of vs and d(vp, rho) = (dvp/dvs, drho/dvs) dvs.  A water layer's Vp and rho are
// constants.  Kind 6 is never asked for.
SD_HD __forceinline__ void closed_forms_dual(int kind, double vs, double dvs, double &vp, double &rho, double &dvp, double &drho)
{
    switch (kind) {
        case 0:  // Sediment
            vp = vs * 2.0;
            rho = 1.22679 + 1.53201 * vs - 0.83668 * vs * vs + 0.20673 * vs * vs * vs - 0.01656 * vs * vs * vs * vs;
            dvp = dvs * 2.0;
            drho = (1.53201 - 2.0 * 0.83668 * vs + 3.0 * 0.20673 * vs * vs - 4.0 * 0.01656 * vs * vs * vs) * dvs; break;
        case 1:  // Crust
            vp = vs * 1.80;
            rho = 1.22679 + 1.53201 * vs - 0.83668 * vs * vs + 0.20673 * vs * vs * vs - 0.01656 * vs * vs * vs * vs;
            dvp = dvs * 1.80;
            drho = (1.53201 - 2.0 * 0.83668 * vs + 3.0 * 0.20673 * vs * vs - 4.0 * 0.01656 * vs * vs * vs) * dvs; break;
        case 2:  // OceanMantle / Mantle
            vp = vs * 1.76; rho = 3.4268 + (vs - 4.5) / 4.5;
            dvp = dvs * 1.76; drho = dvs / 4.5; break;
        case 3:  // OceanWater
            vp = 1.475; rho = 1.027; dvp = 0.0; drho = 0.0; break;
        case 4:  // OceanSediment
        case 7:  // OceanSedimentCascadia = OceanSediment rules
            vp = vs * 1.23 + 1.28; rho = 0.541 + 0.3601 * vp;
            dvp = dvs * 1.23; drho = 0.3601 * dvp; break;
        default: // OceanCrust
            vp = vs * 1.8; rho = 0.541 + 0.3601 * vp;
            dvp = dvs * 1.8; drho = 0.3601 * dvp; break;
    }
}

// grid_value as a dual number for parameter slot j: p the chain's row [random-walk parameters | per-point local constants].
// -max(topo, 0) is a local constant: its slot is never an unknown, z0 carries no derivative.
SD_HD __forceinline__ GridDual grid_value_dual(const int *idesc, const double *fdesc, const double *p, const int g, const int j)
{
    const int nin = idesc[0], ngrid = idesc[1];
    const int *lay_i = idesc + 4;
    const int *coef_i = lay_i + 8 * nin;
    const double *lay_f = fdesc + 1;
    const double *grid_f = lay_f + 9 * nin;

    const double z0 = (lay_i[6] > 0) ? -fmax(p[lay_i[6] - 1], 0.0) : fdesc[0];
    // top zt and thickness Hq of input layer lq with their derivatives; returns the bottom of the last input layer (dzb: its derivative)
    auto layer_span = [&](int lq, double &zt, double &Hq, double &dzt, double &dHq, double &dzb) -> double {
        double z = z0, dz = 0.0;
        zt = z0; Hq = 0.0; dzt = 0.0; dHq = 0.0;
        for (int l = 0; l < nin; ++l) {
            const int hs = lay_i[8 * l + 1];
            double H = (hs >= 0) ? p[hs] : lay_f[9 * l];
            double dH = (hs >= 0 && hs == j) ? 1.0 : 0.0;
            if (lay_i[8 * l + 2]) { H = H - z; dH = dH - dz; }   // BottomDepth: a thickness above enters with the opposite sign
            if (l == lq) { zt = z; Hq = H; dzt = dz; dHq = dH; }
            z += H; dz += dH;
        }
        dzb = dz;
        return z;
    };
    // Vs of grid row gf of input layer l and its derivative: kind 7 the rational function of the thickness, else the basis row
    auto layer_vs = [&](int l, const double *gf, double Hq, double dHq, double &dvs) -> double {
        double vs = 0.0;
        dvs = 0.0;
        if (lay_i[8 * l] == 7) {
            const double H = Hq;
            vs = (0.02 * (H * H) + 1.27 * H + 0.29 * 0.1) / (H + 0.29);
            dvs = ((0.04 * H + 1.27) - vs) / (H + 0.29) * dHq;     // (num' - vs den') / den
        } else {
            const int nc = lay_i[8 * l + 3];
            for (int k = 0; k < nc; ++k) {
                const int sl = coef_i[8 * l + k];
                vs += gf[1 + k] * ((sl >= 0) ? p[sl] : lay_f[9 * l + 1 + k]);
                if (sl >= 0 && sl == j) dvs += gf[1 + k];
            }
        }
        return vs;
    };
    GridDual v;
    double zt, Hq, dzt, dHq, dzb;
    if (g < ngrid) {
        int l = 0;
        while (l + 1 < nin && g >= lay_i[8 * l + 5]) ++l;
        const double *gf = grid_f + 9 * g;
        (void)layer_span(l, zt, Hq, dzt, dHq, dzb);
        v.z = zt + gf[0] * Hq;
        v.dz = dzt + gf[0] * dHq;
        v.vs = layer_vs(l, gf, Hq, dHq, v.dvs);
        closed_forms_dual(lay_i[8 * l], v.vs, v.dvs, v.vp, v.rho, v.dvp, v.drho);
    } else {
        // ReferenceMantle: 21 points hanging off the last grid point - z moves with the bottom, Vs, Vp, rho with that point's
        const int gl = ngrid - 1, l = nin - 1;
        const double *gf = grid_f + 9 * gl;
        const double zref = layer_span(l, zt, Hq, dzt, dHq, dzb);
        double dvs0, vp0, rho0, dvp0, drho0;
        const double vs0 = layer_vs(l, gf, Hq, dHq, dvs0);
        closed_forms_dual(lay_i[8 * l], vs0, dvs0, vp0, rho0, dvp0, drho0);
        const double t = (double)(g - ngrid) / 20.0;
        const double zr = t * 300.0;
        v.z = zref + zr;
        v.vs = vs0 + zr * (0.35 / 200);
        v.vp = vp0 + (v.vs * 1.76 - vs0 * 1.76);
        v.rho = rho0 + ((3.4268 + (v.vs - 4.5) / 4.5) - (3.4268 + (vs0 - 4.5) / 4.5));
        v.dz = dzb;
        v.dvs = dvs0;
        v.dvp = dvp0 + (v.dvs * 1.76 - dvs0 * 1.76);
        v.drho = drho0 + (v.dvs / 4.5 - dvs0 / 4.5);
    }
    return v;
}

// output layer i of the stack (surfdisp_layers_kernel: the midpoint of its two grid points, h = z_b - z_a) as a dual number
SD_HD __forceinline__ LayerDual layer_value_dual(const int *idesc, const double *fdesc, const double *p, const int i, const int j)
{
    const int nin = idesc[0];
    const int *top_i = idesc + 4 + 16 * nin;
    const int g = top_i[i];
    const GridDual a = grid_value_dual(idesc, fdesc, p, g, j), b = grid_value_dual(idesc, fdesc, p, g + 1, j);
    LayerDual o;
    o.v[0] = (a.vp + b.vp) / 2;   o.d[0] = (a.dvp + b.dvp) / 2;
    o.v[1] = (a.vs + b.vs) / 2;   o.d[1] = (a.dvs + b.dvs) / 2;
    o.v[2] = (a.rho + b.rho) / 2; o.d[2] = (a.drho + b.drho) / 2;
    o.v[3] = b.z - a.z;           o.d[3] = b.dz - a.dz;
    return o;
}

}  // namespace sd
