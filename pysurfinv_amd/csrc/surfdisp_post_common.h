// surfdisp_post_common.h -- device helpers the two posterior translation units share: csrc/surfdisp_post.hip (Vs(z) profiles,
// header section (6f)) and csrc/surfdisp_pred.hip (source rows and predictive statistics, section (6g)).
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

}  // namespace sd
