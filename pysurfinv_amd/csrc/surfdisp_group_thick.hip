// surfdisp_group_thick.hip -- K4d of surfdisp_forward_group_thickness_kernels_device (include/surfdisp.h section (5h)): the
// derivatives of the GROUP velocity with respect to the layer thicknesses and the interface depths, combined from the rows the
// thickness kernel (K2e in surfdisp_kernels.hip) wrote at the two shifted periods of K4.  A translation unit of its own: every
// kernel of surfdisp_kernels.hip keeps its instruction stream (profiles/group_thickness/isa_identity.txt).
//
// Rodi's rule of K4 (surfdisp_k_rows.h) holds for any model parameter: here k-, k+ are the rows dcdh of K2e at T (1 - d) and
// T (1 + d), c and U the unit's own values at T; the same for dcdz.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "surfdisp_internal.h"
#include "surfdisp_k_rows.h"

namespace sd {

// K2e's rows are rows already ([B][P][Lmax], transposed by K2e's own 64 x 64 tile), so this is one lane per entry: consecutive
// lanes on consecutive words of every plane, no LDS, no per-thread array; a unit's words (c, U, factors, flags, the first entry
// of each of its three dcdh rows) are the same address across a wavefront or two neighbours.  The unit part of the rule is
// K4c's (rodi_unit, surfdisp_k_rows.h); the four fp32 operations of a result, f1 (km + kp) - f2 (kp - km), are K4c's too, each
// rounded on its own here (contract(off)), whereas K4c's compilation fuses the last two into one fma.  A unit is
//   zeros  where its dcdh at T is zero, entry by entry (dudz[j] goes with dcdh[j - 1], the entry that interface j ends; dudz[0]
//          = 0): below the effective half space at T, beyond nlay, unsolved periods, bad stacks, dudh[nlay - 1];
//   NaN    where K4c writes NaN (a solved unit whose shifted pass failed: counted there), or where one of its three dcdh rows
//          is NaN - K2e marks a unit that is not finite with whole rows of NaN, so the first entry tells; the rows at the
//          shifted periods are looked at only where both shifted roots were found.  Counted here, once per unit.
__global__ __launch_bounds__(256) void surfdisp_group_thick_combine_kernel(GroupThickCombineArgs A)
{
#pragma clang fp contract(off)
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t L = (size_t)A.Lmax;
    if (idx >= (size_t)A.B * A.P * L) return;
    const size_t unit = idx / L;
    const int i = (int)(idx - unit * L);
    const int b = (int)(unit / A.P), k = (int)(unit - (size_t)b * A.P);
    const size_t o = (size_t)k * A.B + b, PB = (size_t)A.P * A.B, row = unit * L;
    float vh = 0.0f, vz = 0.0f;
    const RodiUnit r = rodi_unit(A.ksc0, A.ksc_m, A.ksc_p, A.fail, A.c, A.u, A.inv_dlnT, o, PB);
    if (r.state != RODI_ZEROS) {
        const bool ok = r.state == RODI_COMBINE;
        const float t0 = A.h0[row], tm = A.hm[row], tp = A.hp[row];
        const bool nonfinite = (t0 != t0) || (ok && ((tm != tm) || (tp != tp)));
        if (nonfinite && i == 0 && A.n_nonfinite) atomicAdd(A.n_nonfinite, 1);
        if (!ok || nonfinite) {
            vh = vz = __builtin_nanf("");
        } else {
            if (A.h0[idx] != 0.0f) {
                const float km = A.hm[idx], kp = A.hp[idx];
                vh = r.f1 * (km + kp) - r.f2 * (kp - km);
            }
            if (A.dudz && i > 0 && A.h0[idx - 1] != 0.0f) {
                const float km = A.zm[idx], kp = A.zp[idx];
                vz = r.f1 * (km + kp) - r.f2 * (kp - km);
            }
        }
    }
    A.dudh[idx] = vh;
    if (A.dudz) A.dudz[idx] = vz;
}

hipError_t launch_group_thick_combine(hipStream_t s, const GroupThickCombineArgs &a)
{
    const size_t total = (size_t)a.B * a.P * a.Lmax;
    hipLaunchKernelGGL(surfdisp_group_thick_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
