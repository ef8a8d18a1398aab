// tests/hostcheck/scancheck.hip -- test infrastructure only (tests/test_scan_decide.py).
// Compiles the scan's team decision (pysurfinv_amd/csrc/surfdisp_k_scan.h) for the HOST and runs it, case by case, in its
// four-point form and as two two-point decisions in sequence - the second one from the first one's carry, as two consecutive
// lean passes of the root search do.  Not linked into libsurfdisp_hip.so.
#include <hip/hip_runtime.h>
#include "surfdisp_k_scan.h"
#include <cstdint>
#include <cstring>

static inline int ibits(float v) { int u; memcpy(&u, &v, 4); return u; }

static void put(const sd::ScanOut &o, int *w)
{
    w[0] = o.e; w[1] = o.cross ? 1 : 0;
    w[2] = ibits(o.lo.v); w[3] = ibits(o.lo.c); w[4] = o.lo.mm;
    w[5] = ibits(o.hi.v); w[6] = ibits(o.hi.c); w[7] = o.hi.mm;
}

extern "C" {
// N cases.  v, c, mm: [N][5] = the point before the four (p0) and the four points; g: [N][4] guard flags; first: [N].
// four, seq: [N][8] = event index, crossing, bracket low end / carry (value bits, c bits, mm), high end (the same)
void sc_run(long N, const float *v, const float *c, const int *mm, const int *g, const int *first, int *four, int *seq)
{
    for (long i = 0; i < N; ++i) {
        const float *vi = v + 5 * i, *ci = c + 5 * i;
        const int *mi = mm + 5 * i, *gi = g + 4 * i;
        const sd::ScanPt p0 = {vi[0], ci[0], mi[0], false};
        const sd::ScanPt pt[4] = {{vi[1], ci[1], mi[1], gi[0] != 0}, {vi[2], ci[2], mi[2], gi[1] != 0},
                                  {vi[3], ci[3], mi[3], gi[2] != 0}, {vi[4], ci[4], mi[4], gi[3] != 0}};
        put(sd::scan_decide4(p0, first[i] != 0, pt), four + 8 * i);
        const sd::ScanPt a[2] = {pt[0], pt[1]}, b[2] = {pt[2], pt[3]};
        sd::ScanOut o = sd::scan_decide2(p0, first[i] != 0, a);
        if (o.e < 0) {                                         // the carry is the next pass's previous point; "first" is over
            o = sd::scan_decide2(o.lo, false, b);
            if (o.e >= 0) o.e += 2;
        }
        put(o, seq + 8 * i);
    }
}
}
