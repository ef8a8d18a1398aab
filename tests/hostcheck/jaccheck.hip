// tests/hostcheck/jaccheck.hip -- test infrastructure only (tests/test_param_jacobian_host.py).
// Runs the dual-number statement of the params -> stack map (csrc/surfdisp_layers_dual.h: grid_value_dual, layer_value_dual) on
// the HOST, in the loop order of surfdisp_params_jacobian_kernel: layer [C][4][L] and jac [C][4][L][Nu] of a host descriptor.
// Not linked into libsurfdisp_hip.so.
#include "../../pysurfinv_amd/csrc/surfdisp_layers_dual.h"

extern "C" int sd_jaccheck(int C, int N, int Nu, int L, const double *params, const int *idesc, const double *fdesc, double *layer,
                           double *jac)
{
    if (sd::layers_has_thermal(idesc) || L != idesc[2]) return -1;
    for (int c = 0; c < C; ++c)
        for (int i = 0; i < L; ++i)
            for (int j = 0; j < Nu; ++j) {
                const sd::LayerDual o = sd::layer_value_dual(idesc, fdesc, params + (size_t)c * N, i, j);
                for (int q = 0; q < 4; ++q) {
                    jac[(((size_t)c * 4 + q) * L + i) * Nu + j] = o.d[q];
                    if (j == 0) layer[((size_t)c * 4 + q) * L + i] = o.v[q];
                }
            }
    return 0;
}
