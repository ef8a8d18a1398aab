// surfdisp_post.hip -- posterior Vs(z) profiles of a whole Metropolis track on the device: what the reference's PostPoint
// derives per point (point.py:147-171 the selection, :317-335 _loadValues(zdeps), plotVsProfileShaded / _check_distribution /
// _check_convergency the statistics), for every point of a track [npoints][R][3 + N] at once.  include/surfdisp.h section (6f).
//
// Four launches on the caller's stream:
//   K1 post_select_kernel   one workgroup per (slab of SD_POST_SLAB rows, point): smallest misfit with its first row, last accepted row
//   K2 post_threshold_kernel one thread per point: slabs merged in order -> min_misfit, imin, thres; the accepted row every slab starts from
//   K3 post_profile_kernel  one workgroup per (slab, point, chunk of 64 depths): 256 rows at a time -
//        phase 1 (a thread per row): tile_scan - final test, the row whose parameters count (carried across the tiles and
//        slabs) -, the final rows compacted in row order into LDS with their layer tops;
//        phase 2 (a lane per depth, a wavefront per final row): Vs at the lane's depth from the layer tops, the two bracketing grid
//        points' t and basis rows, and the parameters read from the track IN PLACE; every lane keeps an Acc of its depth in
//        registers (weight 1.0; hist_add for the histogram) - in chunk 0 also of parameter `lane` and `lane + 64`;
//        per slab waves_merge_store.
//   K4 post_finish_kernel   one thread per (point, depth or parameter): slabs_merge, the results written.
// tile_scan, Acc, hist_add, waves_merge_store and slabs_merge are stated in csrc/surfdisp_post_common.h, for this file and
// csrc/surfdisp_pred.hip alike.
// Every sum is fp64 and runs in an order the input alone fixes: two calls give the same bits.  Only the histogram counts are
// integer atomics.  No per-thread array (see surfdisp_mcmc.hip, propose kernel), no scratch, 24 KB of static LDS.
// The arithmetic follows numpy's statement by statement (np.interp: slope * (x - x0) + y0), without contraction to fma.
#include <hip/hip_runtime.h>
#include <math.h>
#include "surfdisp_internal.h"
#include "surfdisp_post_common.h"

#pragma clang fp contract(off)

namespace sd {

constexpr int POST_TOPS = SD_POST_MAX_LAYERS + 1;

// value `sl` of the [params | aux] row of track row `prow`
__device__ __forceinline__ double slot_value(const PostArgs &A, const double *prow, const double *arow, int sl)
{
    return sl < A.N ? prow[3 + sl] : arow[sl - A.N];
}

// Vs at depth zd of the model whose layer tops are tops[0 .. nin] (LDS, stride POST_BLOCK): Model1D.value = np.interp on the grid
// points of seisPropGrids without the reference mantle, NaN outside
__device__ __forceinline__ double vs_at_depth(const PostArgs &A, const double *tops, const double *prow, const double *arow, double zd)
{
    const int nin = A.idesc[0];
    const int *lay_i = A.idesc + 4, *coef_i = lay_i + 8 * nin;
    const double *lay_f = A.fdesc + 1, *grid_f = lay_f + 9 * nin;
    if (!(zd >= tops[0]) || !(zd <= tops[nin * POST_BLOCK])) return NAN;
    int l = 0;                                         // the deepest layer whose top is at or above zd: a doubled interface
    for (int q = 1; q < nin; ++q)                      // point resolves to the lower layer, as np.interp's bracket does
        if (tops[q * POST_BLOCK] <= zd) l = q;
    const double zt = tops[l * POST_BLOCK];
    const int hs = lay_i[8 * l + 1];
    double H = (hs >= 0) ? slot_value(A, prow, arow, hs) : lay_f[9 * l];
    if (lay_i[8 * l + 2]) H = H - zt;                  // BottomDepth
    const int begin = lay_i[8 * l + 4], nint = lay_i[8 * l + 5] - begin - 1;     // grid points begin .. begin + nint
    int j = 0;
    bool at_end = false;
    if (l == nin - 1) at_end = zd >= zt + grid_f[9 * (begin + nint)] * H;        // the last grid depth itself: its value
    if (!at_end) {
        const double f = (zd - zt) / H * (double)nint;                            // t is linspace(0, 1): a guess, then the test itself
        j = f >= (double)(nint - 1) ? nint - 1 : (f > 0.0 ? (int)f : 0);
        while (j > 0 && zt + grid_f[9 * (begin + j)] * H > zd) --j;
        while (j < nint - 1 && zt + grid_f[9 * (begin + j + 1)] * H <= zd) ++j;
    } else {
        j = nint - 1;
    }
    const double *g0 = grid_f + 9 * (begin + j), *g1 = g0 + 9;
    double y0 = 0.0, y1 = 0.0;
    const int kind = lay_i[8 * l];
    if (kind == 7) {                                   // OceanSedimentCascadia
        y0 = y1 = (0.02 * (H * H) + 1.27 * H + 0.29 * 0.1) / (H + 0.29);
    } else {
        const int nc = lay_i[8 * l + 3];
        for (int k = 0; k < nc; ++k) {
            const int sl = coef_i[8 * l + k];
            const double c = (sl >= 0) ? slot_value(A, prow, arow, sl) : lay_f[9 * l + 1 + k];
            y0 += g0[1 + k] * c; y1 += g1[1 + k] * c;
        }
    }
    if (at_end) return y1;
    const double x0 = zt + g0[0] * H, x1 = zt + g1[0] * H;
    const double slope = (y1 - y0) / (x1 - x0);
    return slope * (zd - x0) + y0;
}

__global__ __launch_bounds__(POST_BLOCK) void post_select_kernel(PostArgs A)
{
    __shared__ double s_mis[POST_WAVES];
    __shared__ int s_row[POST_WAVES], s_acc[POST_WAVES];
    const int slab = blockIdx.x % A.nslab, pt = blockIdx.x / A.nslab, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = slab * SD_POST_SLAB, r1 = min(A.R, r0 + SD_POST_SLAB);
    const double *trk = A.track + (size_t)pt * A.R * A.row_stride;
    double mis = INFINITY;
    int row = 0x7fffffff, last = -1;
    for (int r = r0 + tid; r < r1; r += POST_BLOCK) {
        const double *p = trk + (size_t)r * A.row_stride;
        const double m = row_misfit(A, p, r);
        if (min_before(m, r, mis, row)) { mis = m; row = r; }
        if (p[2] > 0.5) last = r;                      // r ascends
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double m2 = __shfl_xor(mis, o);
        const int r2 = __shfl_xor(row, o), l2 = __shfl_xor(last, o);
        if (min_before(m2, r2, mis, row)) { mis = m2; row = r2; }
        last = max(last, l2);
    }
    if (lane == 0) { s_mis[w] = mis; s_row[w] = row; s_acc[w] = last; }
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < POST_WAVES; ++q) {
            if (min_before(s_mis[q], s_row[q], mis, row)) { mis = s_mis[q]; row = s_row[q]; }
            last = max(last, s_acc[q]);
        }
        const size_t k = (size_t)pt * A.nslab + slab;
        A.ws_mis[k] = mis; A.ws_row[k] = row; A.ws_last[k] = last;
    }
}

__global__ __launch_bounds__(64) void post_threshold_kernel(PostArgs A)
{
    const int pt = blockIdx.x * 64 + threadIdx.x;
    if (pt >= A.npoints) return;
    double mis = INFINITY;
    int row = 0x7fffffff, carry = 0;                   // row 0 of a point counts as accepted
    for (int s = 0; s < A.nslab; ++s) {
        const size_t k = (size_t)pt * A.nslab + s;
        A.ws_carry[k] = carry;
        if (min_before(A.ws_mis[k], A.ws_row[k], mis, row)) { mis = A.ws_mis[k]; row = A.ws_row[k]; }
        carry = max(carry, A.ws_last[k]);
    }
    A.min_misfit[pt] = mis;
    A.imin[pt] = row;
    A.thres[pt] = fmax(2.0 * mis, mis + 0.5);
}

__global__ __launch_bounds__(POST_BLOCK) void post_profile_kernel(PostArgs A)
{
    __shared__ double s_buf[POST_TOPS * POST_BLOCK];   // the final rows' layer tops [layer][list entry]; at the slab's end the merge buffer
    __shared__ int s_src[POST_BLOCK];                  // the row whose parameters count, per final row of the tile, in row order
    __shared__ int s_wmax[POST_WAVES], s_wcnt[POST_WAVES];
    const int slab = blockIdx.x % A.nslab, pt = blockIdx.x / A.nslab, chunk = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = slab * SD_POST_SLAB, r1 = min(A.R, r0 + SD_POST_SLAB);
    const double *trk = A.track + (size_t)pt * A.R * A.row_stride;
    const double *arow = A.aux ? A.aux + (size_t)(A.rows ? A.rows[pt] : pt) * A.K : nullptr;
    const double thres = A.thres[pt];
    const int nin = A.idesc[0];
    const int *lay_i = A.idesc + 4;
    const int d = chunk * 64 + lane;
    const bool has_d = d < A.D;
    const double zd = has_d ? A.zdeps[d] : 0.0;
    const bool par = chunk == 0;                       // this workgroup also keeps the parameters' figures
    const bool has_p0 = par && lane < A.N, has_p1 = par && lane + 64 < A.N;
    Acc ad, ap0, ap1;
    acc_clear(ad); acc_clear(ap0); acc_clear(ap1);
    int carry = A.ws_carry[(size_t)pt * A.nslab + slab];
    int nfin = 0;
    for (int t0 = r0; t0 < r1; t0 += POST_BLOCK) {
        // ---- phase 1: a thread per row (tile_scan, csrc/surfdisp_post_common.h); the final rows' sources compacted in row order
        const TileScan ts = tile_scan(A, trk, t0 + tid, r1, thres, carry, s_wmax, s_wcnt);
        const int total = ts.total;
        if (ts.fin) s_src[ts.pos] = ts.src;
        carry = ts.carry;
        nfin += total;
        __syncthreads();
        if (tid < total) {                             // layer tops of final row `tid` of the list: z0, then + H layer by layer
            const double *p = trk + (size_t)s_src[tid] * A.row_stride;
            double z = (lay_i[6] > 0) ? -fmax(slot_value(A, p, arow, lay_i[6] - 1), 0.0) : A.fdesc[0];
            s_buf[tid] = z;
            for (int l = 0; l < nin; ++l) {
                const int hs = lay_i[8 * l + 1];
                double H = (hs >= 0) ? slot_value(A, p, arow, hs) : A.fdesc[1 + 9 * l];
                if (lay_i[8 * l + 2]) H = H - z;
                z += H;
                s_buf[(l + 1) * POST_BLOCK + tid] = z;
            }
        }
        __syncthreads();
        // ---- phase 2: a lane per depth, a wavefront per final row
        for (int j = w; j < total; j += POST_WAVES) {
            const int src = __builtin_amdgcn_readfirstlane(s_src[j]);
            const double *p = trk + (size_t)src * A.row_stride;
            if (has_d) {
                const double v = vs_at_depth(A, s_buf + j, p, arow, zd);
                if (acc_add(ad, v, 1.0) && A.hist)
                    hist_add(A.hist, A.below, A.above, (size_t)pt * A.D + d, A.nbins, v, A.vlo, A.vhi, A.bin_w, A.inv_w, 1);
            }
            if (has_p0) acc_add(ap0, p[3 + lane], 1.0);
            if (has_p1) acc_add(ap1, p[3 + lane + 64], 1.0);
        }
        __syncthreads();
    }
    // ---- the slab's partials: the four wavefronts merged in wavefront order
    const size_t ncol = (size_t)A.D + A.N;
    double *out = A.ws_part + ((size_t)pt * A.nslab + slab) * ncol * 5;
    Part *sp = reinterpret_cast<Part *>(s_buf);        // [wavefront][lane]
    for (int which = 0; which < (par ? 3 : 1); ++which) {
        const Part mine = acc_part(which == 0 ? ad : (which == 1 ? ap0 : ap1));
        sp[w * 64 + lane] = mine;
        __syncthreads();
        const int col = which == 0 ? d : A.D + lane + 64 * (which - 1);
        const bool live = which == 0 ? has_d : (which == 1 ? has_p0 : has_p1);
        if (w == 0 && live) waves_merge_store(sp, lane, out + (size_t)col * 5);
        __syncthreads();
    }
    if (par && tid == 0) A.ws_nfin[(size_t)pt * A.nslab + slab] = nfin;
}

__global__ __launch_bounds__(POST_BLOCK) void post_finish_kernel(PostArgs A)
{
    const int ncol = A.D + A.N;
    const long idx = (long)blockIdx.x * POST_BLOCK + threadIdx.x;
    if (idx >= (long)A.npoints * ncol) return;
    const int pt = (int)(idx / ncol), col = (int)(idx % ncol);
    const Part m = slabs_merge(A.ws_part + ((size_t)pt * A.nslab * ncol + col) * 5, (size_t)ncol * 5, A.nslab);
    if (col == 0) {
        int nfin = 0;
        for (int s = 0; s < A.nslab; ++s) nfin += A.ws_nfin[(size_t)pt * A.nslab + s];
        A.n_final[pt] = nfin;
    }
    const bool any = m.n > 0.0;
    const double mean = any ? m.mean : NAN, sd = any ? sqrt(m.m2 / m.n) : NAN;
    if (col < A.D) {
        const size_t o = (size_t)pt * A.D + col;
        A.count[o] = (int)m.n; A.vs_mean[o] = mean; A.vs_std[o] = sd;
        A.vs_min[o] = any ? m.mn : NAN; A.vs_max[o] = any ? m.mx : NAN;
    } else if (A.pmean) {
        const size_t o = (size_t)pt * A.N + (col - A.D);
        A.pmean[o] = mean; A.pstd[o] = sd;
    }
}

// K1 and K2 alone (also the first two launches of surfdisp_posterior_sources_device, csrc/surfdisp_pred.hip): reads track, R, nslab,
// row_stride, chainL, prefix; writes ws_mis, ws_row, ws_last, ws_carry, min_misfit, imin, thres
hipError_t launch_post_selection(hipStream_t s, const PostArgs &a)
{
    hipLaunchKernelGGL(post_select_kernel, dim3(a.npoints * a.nslab), dim3(POST_BLOCK), 0, s, a);
    hipLaunchKernelGGL(post_threshold_kernel, dim3((a.npoints + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_posterior(hipStream_t s, const PostArgs &a)
{
    const int nchunk = (a.D + 63) / 64;
    const hipError_t e = launch_post_selection(s, a);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(post_profile_kernel, dim3(a.npoints * a.nslab, nchunk), dim3(POST_BLOCK), 0, s, a);
    const long total = (long)a.npoints * (a.D + a.N);
    hipLaunchKernelGGL(post_finish_kernel, dim3((unsigned)((total + POST_BLOCK - 1) / POST_BLOCK)), dim3(POST_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
