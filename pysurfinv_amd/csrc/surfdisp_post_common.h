// surfdisp_post_common.h -- the device pieces the two posterior translation units share: csrc/surfdisp_post.hip (Vs(z) profiles,
// header section (6f)) and csrc/surfdisp_pred.hip (source rows and predictive statistics, section (6g)), each stated once: the
// selection's view of a row, phase 1 of a tile (tile_scan), a column's running figures (Acc), the histogram step (hist_add), and
// the only two merge loops - waves_merge_store (wavefront order within a slab) and slabs_merge (slab order within a point).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "surfdisp_internal.h"

#pragma clang fp contract(off)

namespace sd {

constexpr int POST_BLOCK = 256, POST_WAVES = POST_BLOCK / 64;

__device__ __forceinline__ bool min_before(double ma, int ra, double mb, int rb) { return ma < mb || (ma == mb && ra < rb); }

// misfit of a row as the selection sees it: NaN = +inf, a row outside the prefix = +inf
__device__ __forceinline__ double row_misfit(const PostArgs &A, const double *row, int r)
{
    double m = row[0];
    if (m != m) m = INFINITY;
    if (A.chainL > 0 && (r % A.chainL) >= A.prefix) m = INFINITY;
    return m;
}

// Phase 1 of a tile of POST_BLOCK rows, a thread per row (row r of the point whose track starts at trk; rows at or past r1 take no
// part): is the row final, and which row's parameters count for it - the last accepted row at or before it, or `carry`, the
// one the rows before this tile leave.  An inclusive max-scan over the wavefront, a ballot of the final rows, and one exchange
// of the wavefronts' last accepted rows and final counts through s_wmax / s_wcnt [POST_WAVES].
//   fin    the row is final;  src  the row whose parameters count, max(cand, pre): 0 <= src <= r when carry >= 0
//   pos    the place of a final row among the tile's final rows, in row order;  total  the tile's final rows
//   carry  the carry of the next tile
// Barriers: the ONE inside sits between the write of s_wmax / s_wcnt and their reads.  The caller owns the barrier that keeps the
// next call's write behind this call's reads (every caller has one at the end of its tile), and calls from block-uniform control
// flow only: the tile loop's bound is the same for every thread of the workgroup.
struct TileScan { bool fin; int src, pos, total, carry; };
__device__ __forceinline__ TileScan tile_scan(const PostArgs &A, const double *trk, int r, int r1, double thres, int carry,
                                              int *s_wmax, int *s_wcnt)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    bool fin = false;
    int cand = -1;
    if (r < r1) {
        const double *p = trk + (size_t)r * A.row_stride;
        fin = row_misfit(A, p, r) < thres;
        cand = (!A.tmc || p[2] > 0.5) ? r : -1;
    }
    for (int o = 1; o < 64; o <<= 1) {                 // inclusive max-scan: the last accepted row at or before this one
        const int v = __shfl_up(cand, o);
        if (lane >= o) cand = max(cand, v);
    }
    const unsigned long long bal = __ballot(fin);
    if (lane == 63) s_wmax[w] = cand;
    if (lane == 0) s_wcnt[w] = __popcll(bal);
    __syncthreads();
    int pre = carry, off = 0, total = 0, next = carry;
    for (int q = 0; q < POST_WAVES; ++q) {
        if (q < w) { pre = max(pre, s_wmax[q]); off += s_wcnt[q]; }
        next = max(next, s_wmax[q]); total += s_wcnt[q];
    }
    return TileScan{fin, max(cand, pre), off + (int)__popcll(bal & ((1ull << lane) - 1ull)), total, next};
}

// (n, mean, M2, min, max) of a set of values; n is a count, or a summed integer weight
struct Part { double n, mean, m2, mn, mx; };
// Chan, Golub & LeVeque: b joins a
__device__ __forceinline__ void part_merge(Part &a, const Part &b)
{
    if (b.n == 0.0) return;
    if (a.n == 0.0) { a = b; return; }
    const double n = a.n + b.n, delta = b.mean - a.mean;
    a.mean = a.mean + delta * (b.n / n);
    a.m2 = a.m2 + b.m2 + delta * delta * (a.n * b.n / n);
    a.mn = fmin(a.mn, b.mn); a.mx = fmax(a.mx, b.mx);
    a.n = n;
}

// running figures of one column (a depth, a parameter, a data column) over the rows that count, each with its weight, in row order
struct Acc { double n, piv, s1, s2, mn, mx; };
__device__ __forceinline__ void acc_clear(Acc &a) { a.n = 0.0; a.piv = 0.0; a.s1 = 0.0; a.s2 = 0.0; a.mn = 0.0; a.mx = 0.0; }
// v joins with weight wt > 0 (a whole number; 1.0 for a plain row: 1.0 * d and n += 1.0 are exact) - unless it is not finite:
// THE non-finite rule of a column.  Returns whether v counted, which is also whether it has a place in the histogram.
__device__ __forceinline__ bool acc_add(Acc &a, double v, double wt)
{
    if (!isfinite(v)) return false;
    if (a.n == 0.0) { a.piv = v; a.mn = v; a.mx = v; }
    const double d = v - a.piv;                        // sums about the first value: no cancellation at Vs ~ 4 +- 0.3, c ~ 3.5 +- 0.1
    a.s1 += wt * d; a.s2 += wt * (d * d); a.n += wt;
    a.mn = fmin(a.mn, v); a.mx = fmax(a.mx, v);
    return true;
}
__device__ __forceinline__ Part acc_part(const Acc &a)
{
    Part p{a.n, 0.0, 0.0, a.mn, a.mx};
    if (a.n > 0.0) {
        p.mean = a.piv + a.s1 / a.n;
        const double m2 = a.s2 - a.s1 * a.s1 / a.n;
        p.m2 = m2 > 0.0 ? m2 : 0.0;
    }
    return p;
}

// The histogram step of a finite value v of column `col` ([col] of below / above, [col][nbins] of hist) with integer weight wt:
// below vlo, at or above vhi (!(v < vhi)), or the bin of the edges vlo + i bin_w (np.linspace) - a guess from inv_w, then the
// edges themselves.  Integer atomics: no order.
__device__ __forceinline__ void hist_add(int *hist, int *below, int *above, size_t col, int nbins, double v, double vlo, double vhi,
                                         double bin_w, double inv_w, int wt)
{
    if (v < vlo) atomicAdd(&below[col], wt);
    else if (!(v < vhi)) atomicAdd(&above[col], wt);
    else {
        int b = (int)((v - vlo) * inv_w);
        b = b < 0 ? 0 : (b > nbins - 1 ? nbins - 1 : b);
        if (b > 0 && v < (double)b * bin_w + vlo) --b;
        else if (b < nbins - 1 && v >= (double)(b + 1) * bin_w + vlo) ++b;
        atomicAdd(&hist[col * nbins + b], wt);
    }
}

// The slab's record of column `lane`: the four wavefronts' Parts sp[wavefront][lane] (LDS) merged in wavefront order and stored as
// the five doubles (n, mean, M2, min, max) at o.  For the lanes of wavefront 0; the barrier between the write of sp and this
// call, and the one before sp is written again, are the caller's.
__device__ __forceinline__ void waves_merge_store(const Part *sp, int lane, double *o)
{
    Part m = sp[lane];
    for (int q = 1; q < POST_WAVES; ++q) part_merge(m, sp[q * 64 + lane]);
    o[0] = m.n; o[1] = m.mean; o[2] = m.m2; o[3] = m.mn; o[4] = m.mx;
}

// A point's figures of one column: the records of its nslab slabs, `stride` doubles apart from `first`, merged in slab order
__device__ __forceinline__ Part slabs_merge(const double *first, size_t stride, int nslab)
{
    Part m{0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < nslab; ++s) {
        const double *o = first + (size_t)s * stride;
        part_merge(m, Part{o[0], o[1], o[2], o[3], o[4]});
    }
    return m;
}

}  // namespace sd
