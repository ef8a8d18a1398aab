// surfdisp_k_scan.h -- the scan's team decision over consecutive grid points (phase_body's lean pass, surfdisp_kernels.hip),
// as host + device functions so that a CPU test can walk every pattern (tests/test_scan_decide.py).
//
// The scan (calcul.f:157-170) walks the grid c1, c1 + dc, ... and stops at the first point whose value has another sign than
// the point before it (a bracket: that point and the one before it, each with the layer dropping of its own trial) or that
// fails the guards of calcul.f:165-166 (label 250: the search failed).  A point without either becomes the "previous
// point" of the next one.  A NaN compares as positive.  scan_decide<N> takes N consecutive points at once and returns
// what N single steps would: scan_decide<4> equals two scan_decide<2> in sequence, field for field.
#pragma once
#include "surfdisp_k_common.h"

namespace sd {

struct ScanPt {
    float v, c;      // value of the secular function, trial velocity
    int mm;          // effective half space the value was computed with
    bool g;          // the trial fails a guard of calcul.f:165-166 (counts only without a crossing)
};

struct ScanOut {
    int e;           // first point with a crossing or the guard; -1: none
    bool cross;      // ... a crossing (the bracket is lo, hi); else the guard (label 250)
    ScanPt lo;       // the point before e (p0 for e = 0).  Without an event: the last point - the carry
    ScanPt hi;       // the point e.  Without an event: the last point
};

SD_HD __forceinline__ bool scan_negnan(float x) { return __builtin_signbit(x) && !(x != x); }   // a NaN compares as positive

// crossing or guard of one point against the one before it -> event; *cross: it is a crossing
SD_HD __forceinline__ bool scan_event(float prev_v, bool has_prev, float v, bool g, bool *cross)
{
    *cross = has_prev && (scan_negnan(v) != scan_negnan(prev_v));
    return *cross || (has_prev && g);
}

// p0: the point before pt[0]; first: there is none (a period's first trial)
template <int N>
SD_HD __forceinline__ ScanOut scan_decide(const ScanPt &p0, const bool first, const ScanPt (&pt)[N])
{
    ScanOut o;
    o.e = -1; o.cross = false; o.lo = pt[N - 1]; o.hi = pt[N - 1];
    // from the last point down: the first event in grid order is the one that stays
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        const ScanPt &pv = (i > 0) ? pt[i > 0 ? i - 1 : 0] : p0;
        bool cr;
        if (scan_event(pv.v, (i > 0) || !first, pt[i].v, pt[i].g, &cr)) { o.e = i; o.cross = cr; o.lo = pv; o.hi = pt[i]; }
    }
    return o;
}

SD_HD __forceinline__ ScanOut scan_decide2(const ScanPt &p0, const bool first, const ScanPt (&pt)[2]) { return scan_decide<2>(p0, first, pt); }
SD_HD __forceinline__ ScanOut scan_decide4(const ScanPt &p0, const bool first, const ScanPt (&pt)[4]) { return scan_decide<4>(p0, first, pt); }

}  // namespace sd
