#pragma once
// surfdisp_k_common.h -- what every stage of surfdisp_kernels.hip shares: SD_HD, SD_CERT_STRIDE, the reference's
// constants, the field ids of the staged model and two one-line helpers.
#include "surfdisp_internal.h"

#define SD_HD __host__ __device__
#ifndef SD_CERT_STRIDE
#define SD_CERT_STRIDE 6       // grid points per lane of a certified coarse pass, teams of <= 4 lanes (4: 0.516 ms, 6: 0.483, 8: 0.491 for 65 536 x L10)
#endif

namespace sd {

// ---- reference constants ---------------------------------------------------------------------
constexpr float R0      = 6371.0f;       // flat1.f:21
constexpr float PI_REF  = 3.1415927f;    // calcul.f:32, fast_surf.f:77
constexpr float DC      = 0.01f;         // init.f:25
constexpr float FACT    = 4.0f;          // init.f:25
constexpr float ACCUR   = 1.e-8f;        // surfa.f:191-192
constexpr float CLUSTER_DC = 1.0e-4f;    // spacing of clustered refine points (teams of <= 4 lanes)

// SoA field ids of mdl[NF][Lmax][B]
// (the raw thickness is not staged: nothing downstream reads it, only the flattened one, F_DFL)
enum { F_VP = 0, F_VS, F_RHO, F_QS, F_DIF, F_QQQ, F_DFL, F_HSF, F_HSR, NF = 9 };

SD_HD __forceinline__ bool fin(float x) { return fabsf(x) <= 3.402823466e38f; }   // finite, host+device
SD_HD __forceinline__ float pwr_of(int kind) { return kind == 1 ? 5.0f : 2.2750f; }  // flat1.f:27-28

}  // namespace sd
