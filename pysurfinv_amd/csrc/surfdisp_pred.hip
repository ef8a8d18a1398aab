// surfdisp_pred.hip -- posterior predictive curves of a whole Metropolis track: the two device halves around the forward solve.
// include/surfdisp.h section (6g); pysurfinv_amd.posterior.posterior_predictive drives them.
//
// (1) surfdisp_posterior_sources_device: which rows of a track [npoints][R][3 + N] have to be solved, and how many final rows each
//     stands for.  With trueMarkovChain a rejected row carries the parameters of the last accepted row before it, so the distinct
//     models among the final rows are far fewer than the final rows.  Four launches on the caller's stream:
//       K1, K2 post_select_kernel / post_threshold_kernel of csrc/surfdisp_post.hip (launch_post_selection): min_misfit, imin, thres
//              and the accepted row every slab of SD_POST_SLAB rows starts from (ws_carry)
//       K3 post_sources_kernel  one workgroup per (slab, point), 256 rows at a time, a thread per row - tile_scan
//              (csrc/surfdisp_post_common.h), as phase 1 of post_profile_kernel: the final test and the row whose parameters count,
//              carried across the tiles and slabs; every final row adds 1 to weight[source row] (integer atomics: no order),
//              the thread of row imin writes imin_source, the slab's final rows go to ws_nfin
//       K4 post_sources_count_kernel  one workgroup per point: n_sources = rows with weight > 0, n_final = the slabs' sum
// (2) surfdisp_posterior_predictive_device: weighted column statistics of a list of predictions [total][ld] (float32, P columns
//     used), segmented by point through offsets [npoints + 1].  Two launches (with a histogram K5 is launched once per chunk of 64
//     columns: the per-column ranges travel in the kernel arguments):
//       K5 pred_stats_kernel   one workgroup per (slab, point, chunk of 64 columns): a lane is a column, so the rows of pred are read
//              coalesced; the four wavefronts stride over the rows of the slab.  Every lane keeps the Acc of its column in
//              registers (the profile kernel's, here with the row's integer weight; hist_add for the histogram), then
//              waves_merge_store per slab.  The point's list is cut into slabs of
//              SD_PRED_SLAB rows; workgroup s of the nslab of a point walks slabs s, s + nslab, ... (nslab is fixed by `total`
//              alone), so a list of any length is covered.
//       K6 pred_finish_kernel  one thread per (point, column): slabs_merge, the results written.
// Every sum runs in an order the input alone fixes: two calls give the same bits.  Only the histogram counts are integer atomics
// (adding the row's weight).  No per-thread array, no scratch, LDS only for the merge (10 KB).
// The row loops of K5 hold no barrier: the wavefronts of a workgroup walk different numbers of rows, and every __syncthreads()
// of this file sits outside them (K3's tile loop has a block-uniform bound, its body is predicated).
#include <hip/hip_runtime.h>
#include <math.h>
#include "surfdisp_internal.h"
#include "surfdisp_post_common.h"

#pragma clang fp contract(off)

namespace sd {

__global__ __launch_bounds__(POST_BLOCK) void post_sources_kernel(PostSourcesArgs S)
{
    __shared__ int s_wmax[POST_WAVES], s_wcnt[POST_WAVES];
    const PostArgs &A = S.sel;
    const int slab = blockIdx.x % A.nslab, pt = blockIdx.x / A.nslab, tid = threadIdx.x;
    const int r0 = slab * SD_POST_SLAB, r1 = min(A.R, r0 + SD_POST_SLAB);
    const double *trk = A.track + (size_t)pt * A.R * A.row_stride;
    int *wgt = S.weight + (size_t)pt * A.R;
    const double thres = A.thres[pt];
    const int imin = A.imin[pt];
    int carry = A.ws_carry[(size_t)pt * A.nslab + slab];   // >= 0: row 0 of a point counts as accepted
    int nfin = 0;
    for (int t0 = r0; t0 < r1; t0 += POST_BLOCK) {         // the same bound for every thread of the workgroup
        const int r = t0 + tid;
        const TileScan ts = tile_scan(A, trk, r, r1, thres, carry, s_wmax, s_wcnt);
        if (ts.fin) atomicAdd(&wgt[ts.src], 1);            // 0 <= src <= r
        if (r < r1 && r == imin) S.imin_source[pt] = ts.src;
        carry = ts.carry;
        nfin += ts.total;
        __syncthreads();
    }
    if (tid == 0) A.ws_nfin[(size_t)pt * A.nslab + slab] = nfin;
}

__global__ __launch_bounds__(POST_BLOCK) void post_sources_count_kernel(PostSourcesArgs S)
{
    __shared__ int s_cnt[POST_WAVES];
    const PostArgs &A = S.sel;
    const int pt = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int *wgt = S.weight + (size_t)pt * A.R;
    int n = 0;
    for (int r = tid; r < A.R; r += POST_BLOCK) n += wgt[r] > 0 ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) s_cnt[w] = n;
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < POST_WAVES; ++q) n += s_cnt[q];
        int nfin = 0;
        for (int s = 0; s < A.nslab; ++s) nfin += A.ws_nfin[(size_t)pt * A.nslab + s];
        S.n_sources[pt] = n;
        A.n_final[pt] = nfin;
    }
}

hipError_t launch_post_sources(hipStream_t s, const PostSourcesArgs &a)
{
    const hipError_t e = launch_post_selection(s, a.sel);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(post_sources_kernel, dim3(a.sel.npoints * a.sel.nslab), dim3(POST_BLOCK), 0, s, a);
    hipLaunchKernelGGL(post_sources_count_kernel, dim3(a.sel.npoints), dim3(POST_BLOCK), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(POST_BLOCK) void pred_stats_kernel(PredArgs A)
{
    __shared__ Part s_part[POST_WAVES * 64];               // [wavefront][lane]
    __shared__ int s_fail[POST_WAVES];
    const int slab = blockIdx.x % A.nslab, pt = blockIdx.x / A.nslab, chunk = A.chunk0 + blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = chunk * 64 + lane;
    const bool has = col < A.P;
    const long lo = min(max(A.offsets[pt], 0), A.total), hi = min(max(A.offsets[pt + 1], 0), A.total);   // never outside the list
    const bool hist = A.hist != nullptr && has;
    const double vlo = hist ? A.vlo[lane] : 0.0, vhi = hist ? A.vhi[lane] : 1.0;
    const double bin_w = (vhi - vlo) / A.nbins, inv_w = A.nbins / (vhi - vlo);
    const size_t ocol = (size_t)pt * A.P + col;
    Acc a;
    acc_clear(a);
    int nfail = 0;
    for (long s0 = lo + (long)slab * SD_PRED_SLAB; s0 < hi; s0 += (long)A.nslab * SD_PRED_SLAB) {
        const long s1 = min(hi, s0 + SD_PRED_SLAB);
        for (long j = s0 + w; j < s1; j += POST_WAVES) {   // (no barrier in here: the wavefronts' trip counts differ)
            const int wj = A.w[j];
            if (wj <= 0) continue;
            if (A.failed && A.failed[j]) { nfail += wj; continue; }
            if (!has) continue;
            const double v = (double)A.pred[(size_t)j * A.ld + col];
            if (acc_add(a, v, (double)wj) && hist)
                hist_add(A.hist, A.below, A.above, ocol, A.nbins, v, vlo, vhi, bin_w, inv_w, wj);
        }
    }
    // ---- the workgroup's partials: the four wavefronts merged in wavefront order
    s_part[w * 64 + lane] = acc_part(a);
    if (lane == 0) s_fail[w] = nfail;
    __syncthreads();
    const size_t unit = (size_t)pt * A.nslab + slab;
    if (w == 0 && has) waves_merge_store(s_part, lane, A.ws_part + (unit * A.P + col) * 5);
    if (chunk == 0 && tid == 0) {
        for (int q = 1; q < POST_WAVES; ++q) nfail += s_fail[q];
        A.ws_nfail[unit] = nfail;
    }
}

__global__ __launch_bounds__(POST_BLOCK) void pred_finish_kernel(PredArgs A)
{
    const long idx = (long)blockIdx.x * POST_BLOCK + threadIdx.x;
    if (idx >= (long)A.npoints * A.P) return;
    const int pt = (int)(idx / A.P), col = (int)(idx % A.P);
    const Part m = slabs_merge(A.ws_part + ((size_t)pt * A.nslab * A.P + col) * 5, (size_t)A.P * 5, A.nslab);
    if (col == 0) {
        int nfail = 0;
        for (int s = 0; s < A.nslab; ++s) nfail += A.ws_nfail[(size_t)pt * A.nslab + s];
        A.n_failed[pt] = nfail;
    }
    const bool any = m.n > 0.0;
    A.count[idx] = (int)m.n;
    A.mean[idx] = any ? m.mean : NAN;
    A.std[idx] = any ? sqrt(m.m2 / m.n) : NAN;
    A.mn[idx] = any ? m.mn : NAN;
    A.mx[idx] = any ? m.mx : NAN;
}

hipError_t launch_pred_stats(hipStream_t s, PredArgs a, const double *vlo, const double *vhi)
{
    const int nchunk = (a.P + 63) / 64;
    if (a.hist) {                                          // the ranges travel by value, 64 columns per launch: nothing is read from
        for (int c = 0; c < nchunk; ++c) {                 // the caller's host arrays after the entry returns
            a.chunk0 = c;
            for (int k = 0; k < 64; ++k) {
                const int col = c * 64 + k;
                a.vlo[k] = col < a.P ? vlo[col] : 0.0; a.vhi[k] = col < a.P ? vhi[col] : 1.0;
            }
            hipLaunchKernelGGL(pred_stats_kernel, dim3(a.npoints * a.nslab, 1), dim3(POST_BLOCK), 0, s, a);
        }
    } else {
        a.chunk0 = 0;
        hipLaunchKernelGGL(pred_stats_kernel, dim3(a.npoints * a.nslab, nchunk), dim3(POST_BLOCK), 0, s, a);
    }
    const long total = (long)a.npoints * a.P;
    hipLaunchKernelGGL(pred_finish_kernel, dim3((unsigned)((total + POST_BLOCK - 1) / POST_BLOCK)), dim3(POST_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
