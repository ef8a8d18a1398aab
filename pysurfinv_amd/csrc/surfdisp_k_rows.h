#pragma once
// surfdisp_k_rows.h -- the last step of every analytic-kernel entry: a layer-major scratch [n][Lmax][P][B] (unit index
// un = k*B + b) to the caller's [B][P][Lmax] rows (K2b, K2d, K4c, K5d of surfdisp_kernels.hip), and the unit part of Rodi's
// rule that K4c and K4d (surfdisp_group_thick.hip) share.
#include "surfdisp_k_common.h"

namespace sd {

// One workgroup of 256 lanes moves 64 units x 64 layers through an LDS tile: the scratch is read along the units (a wavefront
// = 64 consecutive words of one layer plane), the rows are written along the layers (a wavefront = 64 consecutive words of one
// unit's row), so both sides are coalesced.  The tile's row stride is 65 words: the fill stores run along a tile row, the
// loads of the store loop down a column whose 64 words fall into 64 different banks.  16 640 bytes of LDS per workgroup.
// Grid: x = P * ceil(B / 64) (period-major: x / ceil(B / 64) is the period), y = ceil(Lmax / 64), z = the kernel's planes.
inline dim3 rows_grid(int B, int P, int Lmax, unsigned planes)
{
    return dim3((unsigned)(P * ((B + 63) / 64)), (unsigned)((Lmax + 63) / 64), planes);
}

// The workgroup's tile and the lane's unit in it: period k, first stack b0, first layer i0, the lane's stack b0 + bl;
// live: b0 + bl < B; un = k * B + b0 + bl, the unit's index in a [P][B] plane (read only where live).
struct RowTile { int k, b0, i0, bl; bool live; size_t un; };

__device__ __forceinline__ RowTile row_tile(int B)
{
    const int nbb = (B + 63) / 64;
    const int k = blockIdx.x / nbb, b0 = (blockIdx.x % nbb) * 64, bl = threadIdx.x % 64;
    return RowTile{k, b0, (int)blockIdx.y * 64, bl, b0 + bl < B, (size_t)k * B + b0 + bl};
}

// value(i) is the entry of the lane's unit at layer i = i0 + il (called for every lane, live or not, and for i >= Lmax: it
// reads nothing where the unit has no entry); rows at or beyond B and layers at or beyond Lmax are not stored.
template <class V>
__device__ __forceinline__ void rows_through_tile(const RowTile &t, int B, int P, int Lmax, float *__restrict__ out, V value)
{
    __shared__ float tile[64][65];
    for (int il = threadIdx.x / 64; il < 64; il += 4) tile[il][t.bl] = value(t.i0 + il);
    __syncthreads();
    for (int q = threadIdx.x; q < 64 * 64; q += 256) {
        const int bq = q / 64, il = q % 64;
        if (t.i0 + il < Lmax && t.b0 + bq < B) out[((size_t)(t.b0 + bq) * P + t.k) * Lmax + t.i0 + il] = tile[il][bq];
    }
}

// Rodi's rule for the derivative of the group velocity with respect to any model parameter m, from the derivatives of the
// phase velocity at T (1 - d) and T (1 + d), k- and k+:
//      dU/dm = (U/c) (2 - U/c) (k- + k+) / 2 - (U/c)^2 (k+ - k-) / ln((1 + d) / (1 - d)) = f1 (k- + k+) - f2 (k+ - k-).
// The unit part: a unit without phase partials at T (factor 0: unsolved) is zeros, a solved unit whose shifted pass failed
// (either root not found, either factor 0, c or U not positive) is NaN, else the two factors.  o = k*B + b, PB = P*B.
enum { RODI_ZEROS = 0, RODI_NAN = 1, RODI_COMBINE = 2 };
struct RodiUnit { int state; float f1, f2; };

SD_HD __forceinline__ RodiUnit rodi_unit(const float *ksc0, const float *ksc_m, const float *ksc_p, const unsigned char *fail,
                                         const float *c, const float *u, float inv_dlnT, size_t o, size_t PB)
{
    if (ksc0[o] == 0.0f) return RodiUnit{RODI_ZEROS, 0.0f, 0.0f};
    // (every word read before the test: a chain of && on the loads themselves makes each wait for the one before it)
    const float cc = c[o], uu = u[o], scm = ksc_m[o], scp = ksc_p[o];
    const bool failed = (fail[o] | fail[PB + o]) != 0;
    const bool ok = !failed && scm != 0.0f && scp != 0.0f && cc > 0.0f && uu > 0.0f;
    if (!ok) return RodiUnit{RODI_NAN, 0.0f, 0.0f};
    const float r = uu / cc;
    return RodiUnit{RODI_COMBINE, 0.5f * r * (2.0f - r),         // (U/c)(2 - U/c) x the mean
                    r * r * inv_dlnT};                            // (U/c)^2 / d ln T
}

}  // namespace sd
