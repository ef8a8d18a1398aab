// surfdisp_capi.hip -- the C ABI of libsurfdisp_hip.so (declared in include/surfdisp.h).
// Host-side only: argument checking, workspace carving, stream-ordered launches.  There is no
// CPU fallback: without a HIP device every entry point fails with SURFDISP_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <cmath>
#include <atomic>
#include "surfdisp_internal.h"

namespace {

thread_local char g_err[512] = "";
// process-wide tuning state (surfdisp_set_team / surfdisp_debug_buffer): atomics, so concurrent callers race
// benignly; a launch reads each value once
std::atomic<int> g_team_override{0};
std::atomic<double *> g_dbg{nullptr};    // developer hook, see surfdisp_debug_buffer

// environment knobs, read ONCE per process (a getenv per launch is visible in launch-bound Metropolis loops)
struct EnvKnobs {
    int team = 0;                 // SURFDISP_TEAM
    int team_love = 0;            // SURFDISP_TEAM_LOVE (developer knob): lanes per stack of Love root searches only
    size_t lds_budget = 44u * 1024u;    // SURFDISP_LDS_BUDGET (developer knob): root-search LDS per 256 lanes
    size_t lds_budget_pipelined = 44u * 1024u;   // SURFDISP_LDS_BUDGET_PIPELINED (developer knob): ... of a SURFDISP_PIPELINED launch (64 KB until r03)
    float refine_wtol = 1.2e-3f;  // SURFDISP_WTOL
    float refine_atol = 1.0e-6f;  // SURFDISP_ATOL
    float ell_ambig = 3.0e-3f;    // SURFDISP_ELL_AMBIG (developer knob): ellipticity closures below this fraction of their terms' magnitude are
                                  // evaluated again with the reference's arithmetic (0 = off)
    float ell_gmax = 25.0f;       // SURFDISP_ELL_GMAX (developer knob): ... and where 2 b^2 / c^2 of the stack's fastest layer exceeds this
    int group_order = -1;         // SURFDISP_GROUP_ORDER (developer knob): workgroup order of the group-velocity kernel (-1: the library's rule; 0: plain period-major; g: XCD-aware, g stack blocks at a time)
    float phimulti = 1.0f;        // SURFDISP_PHIMULTI (developer knob): vertical-phase growth (rad) across a bracket beyond which NEVILL refines it
    bool fastscan = false;        // SURFDISP_FASTSCAN=1: opt every call of the process into the count-guided coarse scan
    int device = 0;               // SURFDISP_DEVICE (fast_surf_)
    int balance = -1;             // SURFDISP_BALANCE (developer knob): wavefront priority by progress, -1 = automatic
    int lockstep = -1;            // SURFDISP_LOCKSTEP (developer knob): -1 = automatic (on), 0 / 1, 2 = also for (stack, period) units
    int certscan = 1;             // SURFDISP_CERTSCAN (developer knob): 0 = Love root searches walk every grid point (no certified skipping)
    int leanscan = 1;             // SURFDISP_LEANSCAN (developer knob): 0 = pure scan passes take the general pass body too
    int host_slots = 3;           // SURFDISP_HOST_SLOTS (developer knob): chunks in flight of a large host-buffer call (2 or 3)
    long host_chunk_layers = 327680;   // SURFDISP_HOST_CHUNK (developer knob): layers' worth of stacks per chunk
    int host_pipeline = 1;        // SURFDISP_HOST_PIPELINE (developer knob): 0 = large host-buffer calls as one chunk
    int rows_min_team = 8;        // SURFDISP_ROWS_MIN_TEAM (developer knob): teams of at least this many lanes rebuild from the row copy
    int group_stash = 1;          // SURFDISP_GROUP_STASH (developer knob): 0 = the Rayleigh group-velocity kernel derives every layer again in each sweep (no LDS stash)
    EnvKnobs()
    {
        if (const char *e = getenv("SURFDISP_TEAM")) team = atoi(e);
        if (const char *e = getenv("SURFDISP_TEAM_LOVE")) team_love = atoi(e);
        if (const char *e = getenv("SURFDISP_LDS_BUDGET")) lds_budget = lds_budget_pipelined = (size_t)atol(e);
        if (const char *e = getenv("SURFDISP_LDS_BUDGET_PIPELINED")) lds_budget_pipelined = (size_t)atol(e);
        if (const char *e = getenv("SURFDISP_WTOL")) refine_wtol = (float)atof(e);
        if (const char *e = getenv("SURFDISP_ATOL")) refine_atol = (float)atof(e);
        if (const char *e = getenv("SURFDISP_PHIMULTI")) phimulti = (float)atof(e);
        if (const char *e = getenv("SURFDISP_GROUP_ORDER")) group_order = atoi(e);
        if (const char *e = getenv("SURFDISP_ELL_AMBIG")) ell_ambig = (float)atof(e);
        if (const char *e = getenv("SURFDISP_ELL_GMAX")) ell_gmax = (float)atof(e);
        if (const char *e = getenv("SURFDISP_FASTSCAN")) fastscan = atoi(e) != 0;
        if (const char *e = getenv("SURFDISP_DEVICE")) device = atoi(e);
        if (const char *e = getenv("SURFDISP_BALANCE")) balance = atoi(e);
        if (const char *e = getenv("SURFDISP_ROWS_MIN_TEAM")) rows_min_team = atoi(e);
        if (const char *e = getenv("SURFDISP_LOCKSTEP")) lockstep = atoi(e);
        if (const char *e = getenv("SURFDISP_HOST_PIPELINE")) host_pipeline = atoi(e);
        if (const char *e = getenv("SURFDISP_CERTSCAN")) certscan = atoi(e);
        if (const char *e = getenv("SURFDISP_LEANSCAN")) leanscan = atoi(e);
        if (const char *e = getenv("SURFDISP_HOST_SLOTS")) host_slots = atoi(e);
        if (const char *e = getenv("SURFDISP_GROUP_STASH")) group_stash = atoi(e);
        if (const char *e = getenv("SURFDISP_HOST_CHUNK")) { host_chunk_layers = atol(e); if (host_chunk_layers < 1024) host_chunk_layers = 1024; }
    }
};
const EnvKnobs &knobs() { static const EnvKnobs k; return k; }

void set_err(const char *fmt, const char *a = "", const char *b = "")
{
    snprintf(g_err, sizeof(g_err), fmt, a, b);
}

#define SD_HIP(call)                                                         \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) {                                              \
            set_err("%s failed: %s", #call, hipGetErrorString(e_));          \
            return SURFDISP_ERR_HIP;                                         \
        }                                                                    \
    } while (0)

constexpr int SD_KIND_FLAGS = SURFDISP_PHASE_ONLY | SURFDISP_INDEPENDENT | SURFDISP_PIPELINED | SURFDISP_EXACTSCAN |
                             SURFDISP_FASTSCAN | SURFDISP_STRICT | SURFDISP_KERN_REFCOORD;

size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// Workspace layout.  A bump carver hands out the arrays of a region one after the other, each padded to 256 bytes; on a null
// base it only counts.  Every region is written once, below, and an entry's workspace is a composition of regions
// (layout()), so a size function and the pointers its entry uses come from the same code.
struct Carver {
    uintptr_t base;
    size_t off;
    explicit Carver(void *b, size_t at = 0) : base(reinterpret_cast<uintptr_t>(b)), off(at) {}
    template <typename T> T *take(size_t count)
    {
        T *p = reinterpret_cast<T *>(base + off);
        off += align_up(count * sizeof(T));
        return p;
    }
};

// the forward solve's region
struct Carve {
    float *mdl, *rows, *ratio, *ct, *ut;
    int *nl, *nsolved, *hist;
    float *fsafe, *ovf;
    int *fb_count, *fb_list;
    int *amb_count;       // [2] brackets sent to NEVILL by the phase rule, ellipticities evaluated again (behind fb_count: zeroed with it)
};
Carve carve(Carver &cv, int B, int Lmax, int P)
{
    const size_t PB = (size_t)P * B;
    Carve c;
    c.mdl = cv.take<float>((size_t)9 * Lmax * B);      // sd::NF staged fields, SoA
    c.rows = cv.take<float>((size_t)9 * Lmax * B);     // ... and one row per stack and field
    c.ratio = cv.take<float>(PB);
    c.ct = cv.take<float>(PB);
    c.ut = cv.take<float>(PB);
    c.hist = cv.take<int>(PB);
    c.nl = cv.take<int>(B);
    c.nsolved = cv.take<int>(B);
    c.fsafe = cv.take<float>(B);
    c.ovf = cv.take<float>((size_t)3 * B);
    c.fb_count = cv.take<int>(3);  c.amb_count = c.fb_count + 1;
    c.fb_list = cv.take<int>(PB);
    return c;
}

// the partials' scratch: layer-major [3][Lmax][P][B] the analytic partials are accumulated in (the lanes of a wavefront -
// consecutive stacks, one period - then touch consecutive words instead of rows 4 P Lmax bytes apart), and per unit its
// factor 1 / (dL/dk) and the deepest layer it wrote
struct KCarve {
    float *kscr, *kscale;
    int *khs;
};
KCarve kcarve(Carver &cv, int B, int Lmax, int P)
{
    const size_t PB = (size_t)P * B;
    KCarve k;
    k.kscr = cv.take<float>((size_t)3 * Lmax * PB);
    k.kscale = cv.take<float>(PB);
    k.khs = cv.take<int>(PB);
    return k;
}

// the group entry's region: a second scratch for T (1 + dfrac) (the partials' scratch, free once the phase partials are
// transposed, takes T (1 - dfrac)), and per shift and unit the factor, deepest layer, root, ellipticity, group velocity and
// failure flag
struct GCarve {
    float *kscr_p, *ksc, *cs, *ratio, *us, *pers;
    int *khs;
    unsigned char *fail;
};
GCarve gcarve(Carver &cv, int B, int Lmax, int P)
{
    const size_t PB = (size_t)P * B;
    GCarve g;
    g.kscr_p = cv.take<float>((size_t)3 * Lmax * PB);
    g.ksc = cv.take<float>(2 * PB);
    g.khs = cv.take<int>(2 * PB);
    g.cs = cv.take<float>(2 * PB);
    g.ratio = cv.take<float>(2 * PB);
    g.us = cv.take<float>(2 * PB);
    g.pers = cv.take<float>((size_t)2 * P);
    g.fail = cv.take<unsigned char>(2 * PB);
    return g;
}

// the ellipticity entry's region: per layer and unit the refreshing period (int), the adjoint row (5 doubles) and the two
// shares (3 + 3 floats), and per unit gamma and the deepest layer
struct ECarve {
    int *kpk;
    double *wscr;
    float *xscr, *fscr, *gam;
    int *khs;
};
ECarve ecarve(Carver &cv, int B, int Lmax, int P)
{
    const size_t PB = (size_t)P * B, LPB = (size_t)Lmax * PB;
    ECarve e;
    e.kpk = cv.take<int>(LPB);
    e.wscr = cv.take<double>(5 * LPB);
    e.xscr = cv.take<float>(3 * LPB);
    e.fscr = cv.take<float>(3 * LPB);
    e.gam = cv.take<float>(PB);
    e.khs = cv.take<int>(PB);
    return e;
}

// the eigenfunction region: the layer-major scratch [4][Lmax][P][B] and per unit the divisor, the deepest layer and the three
// energy integrals
struct EigCarve {
    float *escr, *ediv, *esum;
    int *ehs;
};
EigCarve eigcarve(Carver &cv, int B, int Lmax, int P)
{
    const size_t PB = (size_t)P * B;
    EigCarve e;
    e.escr = cv.take<float>((size_t)4 * Lmax * PB);
    e.ediv = cv.take<float>(PB);
    e.ehs = cv.take<int>(PB);
    e.esum = cv.take<float>(3 * PB);
    return e;
}

// The entries' workspaces: the forward region, then (all but WS_FORWARD and WS_EIGEN) the partials' scratch, then the entry's
// own region(s).  Regions an entry does not have stay null.  The attenuation entry's workspace is WS_KERNELS.
enum WsEntry { WS_FORWARD, WS_KERNELS, WS_GROUP, WS_ELLIP, WS_EIGEN, WS_THICK, WS_GROUP_THICK };
struct Layout {
    Carve w;
    KCarve k;
    GCarve g;
    ECarve e;
    EigCarve eig;
    float *thick_us;      // the thickness entries' plane [P][B]: the U of their EIG group-velocity launches
    float *thick_rows;    // the group-thickness entry's row planes [2 shifts][dcdh, dcdz][B][P][Lmax]: K2e's rows at T (1 -+ dfrac)
    size_t total;
};
Layout layout(void *base, int B, int Lmax, int P, WsEntry entry)
{
    Carver cv(base);
    Layout l{};
    l.w = carve(cv, B, Lmax, P);
    if (entry != WS_FORWARD && entry != WS_EIGEN) l.k = kcarve(cv, B, Lmax, P);
    if (entry == WS_GROUP || entry == WS_GROUP_THICK) l.g = gcarve(cv, B, Lmax, P);
    if (entry == WS_ELLIP) l.e = ecarve(cv, B, Lmax, P);
    if (entry == WS_EIGEN || entry == WS_THICK || entry == WS_GROUP_THICK) l.eig = eigcarve(cv, B, Lmax, P);
    if (entry == WS_THICK || entry == WS_GROUP_THICK) l.thick_us = cv.take<float>((size_t)P * B);
    if (entry == WS_GROUP_THICK) l.thick_rows = cv.take<float>((size_t)4 * B * P * Lmax);
    l.total = cv.off;
    return l;
}
size_t layout_bytes(int B, int Lmax, int P, WsEntry entry)
{
    if (B < 1 || Lmax < 2 || P < 1) return 0;
    return layout(nullptr, B, Lmax, P, entry).total;
}

// The device buffer of one host-buffer batch (a chunk's slot, or the whole call): inputs [model | per | nlay] and outputs
// [c | u | status] contiguous, each padded as the workspace's arrays are, then the forward solve's workspace.
struct HostSlot {
    size_t nm, np, ni, no, ws;                                   // bytes of model, per, nlay = status, c = u, workspace
    size_t o_model, o_per, o_nl, o_c, o_u, o_st, o_ws, bytes;    // their offsets, and the slot's size
    template <typename T> static T *at(char *d, size_t off) { return reinterpret_cast<T *>(d + off); }
};
HostSlot host_slot(int B, int Lmax, int P)
{
    HostSlot h;
    Carver cv(nullptr);
    auto put = [&cv](size_t bytes, size_t &at) { at = cv.off; cv.take<char>(bytes); return bytes; };
    h.nm = put((size_t)B * 5 * Lmax * sizeof(float), h.o_model);
    h.np = put((size_t)P * sizeof(float), h.o_per);
    h.ni = put((size_t)B * sizeof(int), h.o_nl);
    h.no = put((size_t)B * P * sizeof(float), h.o_c);
    put(h.no, h.o_u);
    put(h.ni, h.o_st);
    h.ws = put(layout_bytes(B, Lmax, P, WS_FORWARD), h.o_ws);
    h.bytes = cv.off;
    return h;
}

int pick_team(int B, int Lmax, bool pipelined = false, int kind = SURFDISP_KIND_RAYLEIGH)
{
    int G = g_team_override.load(std::memory_order_relaxed);
    if (G == 0 && kind == SURFDISP_KIND_LOVE) G = knobs().team_love;
    if (G == 0) G = knobs().team;
    if (G == 0) {
        // measured on MI355X (scripts/sweep_team.py, profiles/r02e/sweep_team.txt): at least three wavefronts per
        // SIMD (196 608 lanes on 256 CUs x 4 SIMDs) whatever the batch size, tiny batches a whole wavefront per
        // stack (latency); never fewer than 2 lanes per stack
        const long target = 196608L;
        G = 2;
        while (G < 64 && (long)B * G < target) G *= 2;
        // (r03, with the teams of a wavefront in lock step - profiles/r03b/sweep_team_lockstep.txt: for Rayleigh stacks of
        // >= 24 layers teams of more than 16 lanes cost more in wasted evaluations than the third and fourth wavefront per
        // SIMD give back - 8 192 x L64: 1.49 ms with 16 lanes against 1.68 with 32, 8 192 x L30: 0.76 against 0.84 - so
        // beyond 16 lanes they aim at 131 072 lanes only; and a Rayleigh launch that is alone on the chip never takes
        // two-lane teams - 131 072 x L10: 2.17 against 3.08 ms)
        if (kind != SURFDISP_KIND_LOVE && Lmax >= 24 && G > 16) {
            G = 16;
            while (G < 64 && (long)B * G < 131072L) G *= 2;
        }
        if (kind != SURFDISP_KIND_LOVE && !pipelined && G < 4) G = 4;
    }
    // Love evaluations are cheap (a 2-vector recursion, ~35 instructions per layer against Rayleigh's ~95), so a pass's team
    // bookkeeping weighs more: never fewer than 4 lanes (8 until the teams of a wavefront went in lock step, which took most of
    // that bookkeeping away: 65 536 x L10 now 0.65 ms with 4 lanes against 0.70 with 8, 65 536 x L30 1.46 against 1.55), and
    // the caller sizes a Love launch for its own stacks even beside another stream's kernels (forward_device_impl: 16 384 x L64
    // beside the Rayleigh root search of a joint solve, teams of 16 instead of 8: 6.59 -> 6.24 ms); measured with the four-field
    // Love working stack, scripts/sweep_team.py, profiles/r03a/love_team.txt, profiles/r03b/sweep_team_lockstep.txt
    // (with the certified coarse scan of teams of <= 8 lanes two-lane teams win again on very large batches - 131 072 x L10:
    // 0.73 ms against 0.81 with four lanes - so the floor only holds where that scan is switched off)
    if (kind == SURFDISP_KIND_LOVE && !g_team_override.load(std::memory_order_relaxed) && !knobs().team && !knobs().team_love && G < 4 &&
        knobs().certscan == 0)
        G = 4;
    if (G < 1) G = 1;
    if (G > 64) G = 64;
    int p2 = 1;
    while (p2 * 2 <= G) p2 *= 2;
    G = p2;
    // The working stacks of a workgroup's 256/G teams are what limits the workgroups per CU (one slot each: since r03 the
    // ellipticities of teams of >= 4 lanes come from their own kernel): keep them within 44 KB per 256 lanes, i.e. at least
    // three workgroups = wavefronts per SIMD, normally four - a wider team wastes fewer evaluations than a half-empty SIMD
    // costs (scripts/sweep_team.py,
    // profiles/r02e/sweep_team.txt; re-checked on the r03 kernels, every auto choice within 1 % of the best forced size).
    const size_t per256 = 256 / SD_PHASE_BLOCK;        // the budget is per 256 lanes
    // (until r03 a caller that keeps another batch in flight - SURFDISP_PIPELINED, the joint Rayleigh + Love plan - got 64 KB =
    // two workgroups: the other stream's wavefronts fill the SIMDs, and the narrower team's fewer evaluations won)
    // (r03: with the teams of a wavefront in lock step the wider team wins there too - joint solve of 16 384 x L64, Rayleigh
    // teams of 16 instead of 8: 5.59 -> 5.32 ms - so the budget is the same 44 KB; SURFDISP_LDS_BUDGET_PIPELINED restores 64 KB)
    const size_t budget = pipelined ? knobs().lds_budget_pipelined : knobs().lds_budget;
    auto lds_of = [&](int g) { return sd::phase_lds_bytes(Lmax, g, kind) * per256; };
    while (G < 64 && lds_of(G) > budget) G *= 2;
    return G;
}

int check_args(int B, int Lmax, int P, int kind, const void *model, const void *per,
               const void *c, const void *u)
{
    const int wave = kind & ~SD_KIND_FLAGS;
    if (B < 1 || Lmax < 2 || Lmax > SURFDISP_NLAY_MAX || P < 1 || P > SURFDISP_NPER_MAX ||
        (wave != SURFDISP_KIND_LOVE && wave != SURFDISP_KIND_RAYLEIGH) || !model || !per || !c ||
        (!u && !(kind & SURFDISP_PHASE_ONLY))) {
        set_err("invalid argument (B>=1, 2<=Lmax<=200, 1<=P<=200, kind 1|2, non-null buffers)");
        return SURFDISP_ERR_INVALID;
    }
    return SURFDISP_SUCCESS;
}

}  // namespace

extern "C" {

int surfdisp_abi_version(void) { return SURFDISP_ABI_VERSION; }

const char *surfdisp_last_error(void) { return g_err; }

const char *surfdisp_kernel_name(int which)
{
    switch (which) {
        case 0: return "surfdisp_prep_kernel";
        case 1: return "surfdisp_phase_kernel";
        case 2: return "surfdisp_group_kernel";
        case 3: return "surfdisp_finish_kernel";
        default: return "";
    }
}

int surfdisp_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int surfdisp_set_team(int lanes)
{
    if (lanes < 0 || lanes > 64 || (lanes & (lanes - 1))) {
        set_err("team must be 0 or a power of two <= 64");
        return SURFDISP_ERR_INVALID;
    }
    g_team_override.store(lanes, std::memory_order_relaxed);
    return SURFDISP_SUCCESS;
}

int surfdisp_get_team(int B, int Lmax) { return surfdisp_get_team2(B, Lmax, 1, SURFDISP_KIND_RAYLEIGH); }   // a Rayleigh c+U call, no flags

// lanes per stack a launch with these flags would use (kind: 1 | 2 with SURFDISP_PHASE_ONLY / _PIPELINED / _INDEPENDENT
// OR'd in; P: periods, used by the independent decomposition) - what forward_device_impl computes
int surfdisp_get_team2(int B, int Lmax, int P, int kind)
{
    const bool indep = (kind & SURFDISP_INDEPENDENT) != 0, pipelined = (kind & SURFDISP_PIPELINED) != 0;
    const int wave = kind & ~SD_KIND_FLAGS;
    const long units = (indep ? (long)B * (P > 0 ? P : 1) : (long)B) * ((pipelined && wave != SURFDISP_KIND_LOVE) ? 2 : 1);
    return pick_team((int)(units > 0x3fffffff ? 0x3fffffff : units), Lmax, pipelined, wave);
}

// developer hook (not in include/surfdisp.h): device buffer of B*P*16 doubles receiving
// group-velocity intermediates of the next launches; nullptr switches it off.
void surfdisp_debug_buffer(double *dev) { g_dbg.store(dev, std::memory_order_relaxed); }

// The workspace sizes: each is the end of the composition its entry carves (layout()).  The kernels entry also works, slower,
// on a workspace of only surfdisp_workspace_bytes.
size_t surfdisp_workspace_bytes(int B, int Lmax, int P) { return layout_bytes(B, Lmax, P, WS_FORWARD); }
size_t surfdisp_kernels_workspace_bytes(int B, int Lmax, int P) { return layout_bytes(B, Lmax, P, WS_KERNELS); }
size_t surfdisp_ellip_kernels_workspace_bytes(int B, int Lmax, int P) { return layout_bytes(B, Lmax, P, WS_ELLIP); }
size_t surfdisp_group_kernels_workspace_bytes(int B, int Lmax, int P) { return layout_bytes(B, Lmax, P, WS_GROUP); }
size_t surfdisp_atten_workspace_bytes(int B, int Lmax, int P) { return layout_bytes(B, Lmax, P, WS_KERNELS); }
size_t surfdisp_eigen_workspace_bytes(int B, int Lmax, int P) { return layout_bytes(B, Lmax, P, WS_EIGEN); }
size_t surfdisp_thickness_kernels_workspace_bytes(int B, int Lmax, int P) { return layout_bytes(B, Lmax, P, WS_THICK); }
size_t surfdisp_group_thickness_kernels_workspace_size(int B, int Lmax, int P) { return layout_bytes(B, Lmax, P, WS_GROUP_THICK); }

// developer / test read-out (not in include/surfdisp.h): byte offset, inside that workspace, of the shifted roots
// [2][P][B] (float; T (1 - dfrac) first) of the last surfdisp_forward_group_kernels_device call on it
size_t surfdisp_group_kernels_shift_offset(int B, int Lmax, int P)
{
    if (B < 1 || Lmax < 2 || P < 1) return 0;
    return (size_t)reinterpret_cast<uintptr_t>(layout(nullptr, B, Lmax, P, WS_GROUP).g.cs);   // (null base: the pointer is the offset)
}

// test read-out (not in include/surfdisp.h): byte offsets, inside a forward workspace, of what the prep kernel writes - the SoA copy
// mdl [9][Lmax][B], the row copy rows [B][9][Lmax], nl [B], fsafe [B], ovf [3][B] (float / int words).  0 on success.
int surfdisp_workspace_prep_offsets(int B, int Lmax, int P, size_t out[5])
{
    if (B < 1 || Lmax < 2 || P < 1 || !out) return SURFDISP_ERR_INVALID;
    const Carve w = layout(nullptr, B, Lmax, P, WS_FORWARD).w;                  // (null base: a pointer is its offset)
    out[0] = (size_t)reinterpret_cast<uintptr_t>(w.mdl);
    out[1] = (size_t)reinterpret_cast<uintptr_t>(w.rows);
    out[2] = (size_t)reinterpret_cast<uintptr_t>(w.nl);
    out[3] = (size_t)reinterpret_cast<uintptr_t>(w.fsafe);
    out[4] = (size_t)reinterpret_cast<uintptr_t>(w.ovf);
    return SURFDISP_SUCCESS;
}

// introspection: n words from fb_count on of the last solve that used this workspace.  Waits for `stream`.
static int read_counters(void *stream, const void *workspace, int B, int Lmax, int P, int *counts, int n)
{
    if (!workspace || !counts || B < 1 || Lmax < 2 || P < 1) { set_err("bad argument"); return SURFDISP_ERR_INVALID; }
    const Carve w = layout(const_cast<void *>(workspace), B, Lmax, P, WS_FORWARD).w;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SD_HIP(hipMemcpyAsync(counts, w.fb_count, n * sizeof(int), hipMemcpyDeviceToHost, s));
    SD_HIP(hipStreamSynchronize(s));
    return SURFDISP_SUCCESS;
}

// how many stacks (or (stack, period) units in independent mode) the solve handed to the exact fallback kernel
int surfdisp_workspace_fallback_count(void *stream, const void *workspace, int B, int Lmax, int P, int *count) { return read_counters(stream, workspace, B, Lmax, P, count, 1); }

// {stacks handed to the exact fallback kernel, brackets sent to NEVILL because the vertical phase grows by more than
// SURFDISP_PHIMULTI across them, ellipticities evaluated again with the reference's arithmetic}
int surfdisp_workspace_counters(void *stream, const void *workspace, int B, int Lmax, int P, int *counts3) { return read_counters(stream, workspace, B, Lmax, P, counts3, 3); }

// What a caller of forward_device_impl asks for beyond c, u and status.
struct ForwardOpts {
    hipEvent_t *events = nullptr;         // four events, recorded before prep, between the kernels and after finish
    float *dcdb = nullptr, *dcda = nullptr, *dcdr = nullptr;   // rows [B][P][Lmax] of the analytic partials of c (dcdb switches them on)
    float *ratio = nullptr;               // the caller's ellipticity array [B][P]
    bool record_history = false;          // record the refresh history also where the solve itself needs none (the ellipticity kernels replay it)
    bool keep_vp_plane = false;           // keep the dc/dVp plane in the partials' scratch also without dcda rows (the attenuation kernel reads it)
    bool keep_rho_plane = false;          // ... and the dc/drho plane without dcdr rows (the thickness kernel)
    const EigCarve *eigen = nullptr;      // the eigen region: the group-velocity kernel's EIG instantiation fills it
};

static int forward_device_impl(void *stream, int B, int Lmax, const int *nlay,
                               const float *model, int P, const float *per, int kind,
                               float *c, float *u, int *status,
                               void *workspace, size_t workspace_bytes, const ForwardOpts &o)
{
    hipEvent_t *const ev = o.events;
    float *const kb = o.dcdb, *const ka = o.dcda, *const kr = o.dcdr, *const ratio = o.ratio;
    int rc = check_args(B, Lmax, P, kind, model, per, c, u);
    if (rc) return rc;
    if (!workspace || workspace_bytes < surfdisp_workspace_bytes(B, Lmax, P)) {
        set_err("workspace too small");
        return SURFDISP_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool phase_only = (kind & SURFDISP_PHASE_ONLY) != 0;
    const bool indep = (kind & SURFDISP_INDEPENDENT) != 0;
    const bool pipelined = (kind & SURFDISP_PIPELINED) != 0;
    // the reference's point-by-point scan unless the caller (flag) or the process (environment) opted into the
    // count-guided coarse one; SURFDISP_EXACTSCAN (ABI 1) is accepted and wins over both
    const EnvKnobs &kn = knobs();
    const bool strict = (kind & SURFDISP_STRICT) != 0;
    const bool exactscan = (kind & SURFDISP_EXACTSCAN) != 0;
    const bool kern_raw = (kind & SURFDISP_KERN_REFCOORD) != 0;
    bool fastscan = ((kind & SURFDISP_FASTSCAN) != 0 || kn.fastscan) && !exactscan && !strict;
    kind &= ~SD_KIND_FLAGS;
    // Love: the coarse scan with its Sturm-count certificate (phase_body, CERT) is the DEFAULT - it returns the bracket the
    // point-by-point scan returns, by a theorem, not a heuristic; SURFDISP_EXACTSCAN / SURFDISP_CERTSCAN=0 walk every point
    if (kind == SURFDISP_KIND_LOVE) fastscan = !exactscan && !strict && (kn.certscan != 0 || fastscan);
    // the ellipticity recursions (two more evaluations per period) feed the group-velocity kernel - and the caller who
    // asked for the ratio itself (ABI 3), also in a phase-only call
    const bool want_ell = (kind == SURFDISP_KIND_RAYLEIGH) && (!phase_only || ratio != nullptr);
    const Layout lay = layout(workspace, B, Lmax, P, WS_KERNELS);
    const Carve &w = lay.w;
    // independent mode has B*P root searches in flight: size the teams for that many; a caller that
    // keeps a second batch in flight (SURFDISP_PIPELINED) has twice the stacks on the chip
    const long units = (indep ? (long)B * P : (long)B) * ((pipelined && kind != SURFDISP_KIND_LOVE) ? 2 : 1);
    // The ellipticities come from their own kernel (one lane per (stack, period), replaying the working stack's history):
    // the root search then runs as in a phase-only call - no riders, no second LDS slot.  The exact fallback kernel
    // (and SURFDISP_STRICT) keeps them in-kernel.
    // Teams of two lanes keep them too: their ellipticity pass has both lanes busy, one start vector each (three batches in
    // flight, 65 536 x L10: 34.0 M solves/s in-kernel against 33.6 M with the extra kernel).
    const bool ell_k_ok = want_ell && !strict;
    const int G = pick_team((int)(units > 0x3fffffff ? 0x3fffffff : units), Lmax, pipelined, kind);
    const bool ell_k = ell_k_ok && G >= 4;
    const bool ell_in = want_ell && !ell_k;

    // Staged copy of the model the root search rebuilds its working stack from, once per period: with >= 8 lanes per
    // stack consecutive lanes take consecutive layers, so the fields are laid out one row per stack (coalesced; from the
    // SoA copy every value costs its own cache line: 12.5 GB of fabric traffic per 25 600 x 96-layer lock step,
    // profiles/r03a).  Narrow teams read the SoA copy (consecutive stacks share a line).  The group-velocity kernel - one
    // lane per (stack, period) - always reads the SoA copy; a phase-only call with rows skips writing it (the exact
    // fallback launch reads whatever the production launch read).
    const bool use_rows = (G >= kn.rows_min_team);
    const bool need_soa = !use_rows || !phase_only || want_ell;
    sd::PrepArgs pa{B, Lmax, nlay, model, w.mdl, w.nl, P, indep ? w.nsolved : nullptr, w.fsafe, w.ovf, w.fb_count,
                    use_rows ? w.rows : nullptr, need_soa ? 1 : 0};
    if (ev) SD_HIP(hipEventRecord(ev[0], s));
    SD_HIP(sd::launch_prep(s, kind, pa));
    if (ev) SD_HIP(hipEventRecord(ev[1], s));
    const float wtol = kn.refine_wtol, atol = kn.refine_atol;
    sd::PhaseArgs ph{B, Lmax, P, w.mdl, w.nl, per, w.ct, ell_in ? w.ratio : nullptr, w.nsolved, status, wtol, atol,
                     fastscan ? 1 : 0, w.fsafe, /* overlap, phimax: layout only */ 0, 0.0f, w.ovf, w.fb_count, w.fb_list, kn.balance >= 0 ? kn.balance : ((pipelined && G < 8) ? 0 : 1), strict ? 1 : 0};
#ifdef SD_WAVECLOCK
    ph.wclk = reinterpret_cast<unsigned long long *>(g_dbg.load(std::memory_order_relaxed));
#endif
    if (use_rows) { ph.msrc = w.rows; ph.ms_b = 9L * Lmax; ph.ms_f = Lmax; ph.ms_i = 1; }
    else          { ph.msrc = w.mdl;  ph.ms_b = 1;         ph.ms_f = (long)Lmax * B; ph.ms_i = B; }
    // (two-lane teams compute their ellipticities themselves but record the history too: the pairs whose closure cancels
    // are redone by the ellipticity kernel)
    const bool ell_fix = ell_in && !strict && kn.ell_ambig != 0.0f;
    ph.hist = (ell_k || ell_fix || o.record_history) ? w.hist : nullptr;
    ph.lockstep = kn.lockstep >= 0 ? kn.lockstep : 1;
    ph.phimulti = kn.phimulti; ph.amb_count = w.amb_count; ph.ell_ambig = ell_fix ? kn.ell_ambig : 0.0f; ph.ell_gmax = kn.ell_gmax;
    ph.scan_general = kn.leanscan ? 0 : 1;
    SD_HIP(sd::launch_phase(s, kind, G, indep, ph));
    // the exact fallback re-solves what the production kernel listed (normally nothing: idle blocks exit at once)
    ph.fast = 0;
    if (ell_k) ph.ratio = w.ratio;                         // ... with its ellipticities in-kernel (marked -1 in hist)
    SD_HIP(sd::launch_phase_exact(s, kind, indep, ph));
    if (ev) SD_HIP(hipEventRecord(ev[2], s));              // [ev1, ev2] = the root search (+ its idle fallback launch)
    if (ell_k || ell_fix) {
        sd::EllipArgs ea{B, Lmax, P, w.mdl, w.nl, per, w.ct, w.hist, w.nsolved, w.ratio, kn.ell_ambig, ell_k ? 0 : 1, w.amb_count, kn.ell_gmax, w.ovf};
        SD_HIP(sd::launch_ellip(s, ea));
    }
#ifdef SD_WAVECLOCK
    double *gdbg = nullptr;                                // the debug buffer holds wavefront clocks in this build
#else
    double *gdbg = g_dbg.load(std::memory_order_relaxed);
#endif
    // analytic partials: through the layer-major scratch when the caller's workspace has room for it
    float *kscr = nullptr, *kscale = nullptr;
    int *khs = nullptr;
    if (kb && workspace_bytes >= lay.total) { kscr = lay.k.kscr; kscale = lay.k.kscale; khs = lay.k.khs; }
    // (on the scratch route kb / ka / kr only say which planes the kernel stores: keep_vp_plane / keep_rho_plane ask for a
    // plane also when the caller wants no rows of it)
    sd::GroupArgs ga{B, Lmax, P, w.mdl, w.nl, per, w.ct, w.ratio, w.nsolved, w.ut, gdbg, kb, (o.keep_vp_plane && kscr && !ka) ? kb : ka,
                     (o.keep_rho_plane && kscr && !kr) ? kb : kr,
                     kscr, kscale, khs, kern_raw ? 1 : 0, 0, 0, kn.group_order};
    if (o.eigen) { ga.escr = o.eigen->escr; ga.ediv = o.eigen->ediv; ga.ehs = o.eigen->ehs; ga.esum = o.eigen->esum; }   // (the EIG instantiation)
    // (not beside other batches: the stash's 50 KB per workgroup would keep their root-search workgroups off the CU)
    ga.stash = (kn.group_stash && !pipelined) ? 0 : -1;
    if (!phase_only) SD_HIP(sd::launch_group(s, kind, ga));
    if (!phase_only && kscr) {
        // one launch for the three arrays: factor 1 / (dL/dk), zeros below each unit's half space, whole rows
        sd::KernTransposeArgs ta{B, P, Lmax, kind, kscr, kscale, khs, kb, ka, kr};
        SD_HIP(sd::launch_kern_transpose(s, ta));
    }
    if (ratio && kind != SURFDISP_KIND_RAYLEIGH) SD_HIP(hipMemsetAsync(ratio, 0, (size_t)B * P * sizeof(float), s));   // Love: zeros
    sd::FinishArgs fa{B, P, w.ct, phase_only ? nullptr : w.ut, c, phase_only ? nullptr : u,
                      indep ? w.nsolved : nullptr, w.nl, status,
                      (ratio && want_ell) ? w.ratio : nullptr, (ratio && want_ell) ? ratio : nullptr, w.nsolved};
    SD_HIP(sd::launch_finish(s, fa));
    if (ev) SD_HIP(hipEventRecord(ev[3], s));
    return SURFDISP_SUCCESS;
}

int surfdisp_forward_batch_device(void *stream, int B, int Lmax, const int *nlay,
                                  const float *model, int P, const float *per, int kind,
                                  float *c, float *u, int *status,
                                  void *workspace, size_t workspace_bytes)
{
    return forward_device_impl(stream, B, Lmax, nlay, model, P, per, kind, c, u, status,
                               workspace, workspace_bytes, ForwardOpts());
}

// ABI 3: the same solve, also returning the Rayleigh ellipticity the reference keeps in COMMON /o/ (calcul.f:195).
int surfdisp_forward_batch_device2(void *stream, int B, int Lmax, const int *nlay,
                                   const float *model, int P, const float *per, int kind,
                                   float *c, float *u, float *ratio, int *status,
                                   void *workspace, size_t workspace_bytes)
{
    ForwardOpts o;
    o.ratio = ratio;
    return forward_device_impl(stream, B, Lmax, nlay, model, P, per, kind, c, u, status,
                               workspace, workspace_bytes, o);
}

// The preamble of the entries below, in the order each performs it: required pointers (`have`; `required` names them in the
// error text), refused kind flags, the entry's own extra test (`extra`: its error text where it failed, else null), check_args,
// workspace size.  `ws`: the composition the entry needs at least, `ws_fn` the size function the error text names (null: none),
// `ws_rc` the return code for a smaller workspace (it differs between the entries).
static int entry_preamble(const char *name, bool have, const char *required, int refused, const char *refused_text,
                          const char *extra, int B, int Lmax, int P, int kind, const void *model, const void *per,
                          const void *c, const void *u, const void *workspace, size_t workspace_bytes, WsEntry ws,
                          const char *ws_fn, int ws_rc)
{
    if (!have) { set_err("%s: %s is NULL", name, required); return SURFDISP_ERR_INVALID; }
    if (kind & refused) { set_err("%s: %s", name, refused_text); return SURFDISP_ERR_INVALID; }
    if (extra) { set_err("%s: %s", name, extra); return SURFDISP_ERR_INVALID; }
    int rc = check_args(B, Lmax, P, kind, model, per, c, u);
    if (rc) return rc;
    if (workspace && workspace_bytes >= layout_bytes(B, Lmax, P, ws)) return SURFDISP_SUCCESS;
    set_err(ws_fn ? "workspace too small (%s)" : "workspace too small", ws_fn ? ws_fn : "");
    return ws_rc;
}

// Forward solve + analytic partial derivatives of the phase velocity with respect to each layer's
// Vs, Vp, rho (what REIGEN/LEIGEN compute and discard, surfa.f:1130-1135,1204-1207 /
// 561-565,584-585), from the energy integrals the group-velocity kernel forms anyway.
int surfdisp_forward_kernels_device(void *stream, int B, int Lmax, const int *nlay,
                                    const float *model, int P, const float *per, int kind,
                                    float *c, float *u, int *status,
                                    float *dcdb, float *dcda, float *dcdr,
                                    void *workspace, size_t workspace_bytes)
{
    // (a workspace of only the forward solve's size is accepted: the direct route into the rows)
    int rc = entry_preamble("surfdisp_forward_kernels_device", dcdb != nullptr, "dcdb", SURFDISP_PHASE_ONLY,
                            "the partials come from the group-velocity kernel (no PHASE_ONLY)", nullptr, B, Lmax, P, kind, model, per,
                            c, u, workspace, workspace_bytes, WS_FORWARD, nullptr, SURFDISP_ERR_WORKSPACE);
    if (rc) return rc;
    ForwardOpts o;
    o.dcdb = dcdb; o.dcda = dcda; o.dcdr = dcdr;
    return forward_device_impl(stream, B, Lmax, nlay, model, P, per, kind, c, u, status, workspace, workspace_bytes, o);
}

// The thickness pass of the two thickness entries: the EIG instantiation of the group-velocity kernel (kb = nullptr: it writes
// no partials; its U goes to the scratch plane) on the roots `tc` and ellipticities `tratio` at the periods `tper`, then K2e on
// the eigen region it filled and the given KERN scratch (`tkscr`, factors `tksc`, deepest layers `tkhs`) with the group
// velocities `tu` -> the rows dh, dz (dz may be nullptr).  n_nonfinite: nullptr, or where K2e counts the units that are not finite.
static int thickness_pass(hipStream_t s, int B, int Lmax, int P, int wave, const float *model, const Layout &lay,
                          const float *tper, const float *tc, const float *tratio, const float *tu, const float *tkscr,
                          const float *tksc, const int *tkhs, float *dh, float *dz, int *n_nonfinite)
{
    const Carve &w = lay.w;
    const EigCarve &e = lay.eig;
    sd::GroupArgs ga{B, Lmax, P, w.mdl, w.nl, tper, tc, tratio, w.nsolved, lay.thick_us, nullptr, nullptr, nullptr, nullptr,
                     nullptr, nullptr, nullptr, 0, 0, 0, knobs().group_order};
    ga.escr = e.escr; ga.ediv = e.ediv; ga.ehs = e.ehs; ga.esum = e.esum;
    ga.stash = -1;
    SD_HIP(sd::launch_group(s, wave, ga));
    sd::ThickArgs ta{B, P, Lmax, wave, model, w.mdl, w.nl, tper, e.escr, e.ediv, e.ehs, e.esum, tkscr, tksc, tkhs,
                     tc, tu, dh, dz, n_nonfinite};
    SD_HIP(sd::launch_thickness(s, ta));
    return SURFDISP_SUCCESS;
}

// What surfdisp_forward_group_thickness_kernels_device asks of group_launches beyond the group entry's outputs.
struct GroupThickOuts {
    float *dcdh, *dcdz, *dudh, *dudz;     // the caller's [B][P][Lmax] rows (dcdz, dudz may be nullptr)
    int *n_nonfinite;
};

// The launches of the two group entries behind their preambles.  `ws`: the entry's workspace composition; `t`: null for the
// group entry.  With `t` the thickness passes run where their inputs are still (or already) in the scratches: K2e at T before
// the shifted KERN launch of shift 0 overwrites the phase partials' scratch, K2e at a shifted period right behind that shift's
// KERN launch (its scratch, factor, deepest layer and U) and an EIG launch on the same root into the one eigen region.  They
// read what the group entry's launches write and write only the eigen region, the U plane, the row planes and the caller's
// thickness rows, so c .. dudr are the group entry's; the shifted KERN launches keep the dc/dVp and dc/drho planes whether or
// not the caller wants duda / dudr rows (K2e reads them), which changes no value of a plane.
static int group_launches(void *stream, int B, int Lmax, const int *nlay, const float *model, int P, const float *per, int kind,
                          float dlnT_frac, float *c, float *u, int *status, float *dcdb, float *dcda, float *dcdr,
                          float *dudb, float *duda, float *dudr, int *n_shift_failed, void *workspace, size_t workspace_bytes,
                          WsEntry ws, const GroupThickOuts *t)
{
    ForwardOpts o;
    o.dcdb = dcdb; o.dcda = dcda; o.dcdr = dcdr;
    if (t) o.keep_vp_plane = o.keep_rho_plane = true;
    int rc = forward_device_impl(stream, B, Lmax, nlay, model, P, per, kind, c, u, status, workspace, workspace_bytes, o);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int wave = kind & ~SD_KIND_FLAGS;
    const EnvKnobs &kn = knobs();
    const Layout lay = layout(workspace, B, Lmax, P, ws);
    const Carve &w = lay.w;
    const GCarve &g = lay.g;
    const size_t PB = (size_t)P * B, rows = PB * Lmax;
    float *kscr = lay.k.kscr, *kscale0 = lay.k.kscale;                           // forward_device_impl's scratch and factors
    if (t) {
        if (t->n_nonfinite) SD_HIP(hipMemsetAsync(t->n_nonfinite, 0, sizeof(int), s));
        // (a NaN row marks a unit that is not finite; the combination counts them)
        rc = thickness_pass(s, B, Lmax, P, wave, model, lay, per, w.ct, w.ratio, w.ut, kscr, kscale0, lay.k.khs, t->dcdh, t->dcdz,
                            nullptr);
        if (rc) return rc;
    }
    if (n_shift_failed) SD_HIP(hipMemsetAsync(n_shift_failed, 0, sizeof(int), s));
    sd::ShiftArgs sa{B, Lmax, P, wave, w.mdl, w.nl, per, w.ct, w.ut, w.nsolved, dlnT_frac, g.pers, g.cs,
                     wave == SURFDISP_KIND_RAYLEIGH ? g.ratio : nullptr, g.fail, kn.ell_ambig, kn.ell_gmax, w.ovf};
    SD_HIP(sd::launch_shift(s, sa));
    // the row planes: [shift][dcdh, dcdz][B][P][Lmax]
    auto plane = [&](int sg, int z) { return lay.thick_rows + (size_t)(2 * sg + z) * rows; };
    for (int sg = 0; sg < 2; ++sg) {
        // (kb / ka / kr only say which partials are wanted: on the scratch route the kernel writes the scratch alone)
        float *const ka = wave == SURFDISP_KIND_RAYLEIGH ? (t ? dudb : duda) : nullptr, *const kr = t ? dudb : dudr;
        sd::GroupArgs ga{B, Lmax, P, w.mdl, w.nl, g.pers + (size_t)sg * P, g.cs + sg * PB, g.ratio + sg * PB, w.nsolved,
                         g.us + sg * PB, nullptr, dudb, ka, kr,
                         sg ? g.kscr_p : kscr, g.ksc + sg * PB, g.khs + sg * PB, 0, 0, 0, kn.group_order};
        SD_HIP(sd::launch_group(s, wave, ga));
        if (t) {
            rc = thickness_pass(s, B, Lmax, P, wave, model, lay, g.pers + (size_t)sg * P, g.cs + sg * PB, g.ratio + sg * PB,
                                g.us + sg * PB, sg ? g.kscr_p : kscr, g.ksc + sg * PB, g.khs + sg * PB, plane(sg, 0),
                                t->dudz ? plane(sg, 1) : nullptr, nullptr);
            if (rc) return rc;
        }
    }
    const float inv_dlnT = (float)(1.0 / log((1.0 + (double)dlnT_frac) / (1.0 - (double)dlnT_frac)));
    sd::GroupCombineArgs ca{B, P, Lmax, wave, kscr, g.kscr_p, g.ksc, g.ksc + PB, g.khs, g.khs + PB, kscale0, g.fail,
                            w.ct, w.ut, inv_dlnT, dudb, duda, dudr, n_shift_failed};
    SD_HIP(sd::launch_group_combine(s, ca));
    if (t) {
        sd::GroupThickCombineArgs ta{B, P, Lmax, plane(0, 0), plane(1, 0), plane(0, 1), plane(1, 1), t->dcdh, g.ksc, g.ksc + PB,
                                     kscale0, g.fail, w.ct, w.ut, inv_dlnT, t->dudh, t->dudz, t->n_nonfinite};
        SD_HIP(sd::launch_group_thick_combine(s, ta));
    }
    return SURFDISP_SUCCESS;
}

// The same launches, then the analytic partials of the GROUP velocity (K4 in surfdisp_kernels.hip): the roots at
// T (1 -+ dlnT_frac), the phase partials there, and their combination.  c, u, status, dc* are those of
// surfdisp_forward_kernels_device, bit for bit.
int surfdisp_forward_group_kernels_device(void *stream, int B, int Lmax, const int *nlay,
                                          const float *model, int P, const float *per, int kind, float dlnT_frac,
                                          float *c, float *u, int *status,
                                          float *dcdb, float *dcda, float *dcdr,
                                          float *dudb, float *duda, float *dudr, int *n_shift_failed,
                                          void *workspace, size_t workspace_bytes)
{
    int rc = entry_preamble("surfdisp_forward_group_kernels_device", dcdb && dudb, "dcdb or dudb",
                            SURFDISP_PHASE_ONLY | SURFDISP_KERN_REFCOORD, "no PHASE_ONLY, no KERN_REFCOORD",
                            (dlnT_frac >= 1.0e-3f && dlnT_frac <= 0.05f) ? nullptr : "dlnT_frac outside [1e-3, 0.05]",
                            B, Lmax, P, kind, model, per, c, u, workspace, workspace_bytes, WS_GROUP,
                            "surfdisp_group_kernels_workspace_bytes", SURFDISP_ERR_WORKSPACE);
    if (rc) return rc;
    return group_launches(stream, B, Lmax, nlay, model, P, per, kind, dlnT_frac, c, u, status, dcdb, dcda, dcdr, dudb, duda, dudr,
                          n_shift_failed, workspace, workspace_bytes, WS_GROUP, nullptr);
}

// The same launches as surfdisp_forward_kernels_device (c, u, status, dc* bit for bit; `ratio` as
// surfdisp_forward_batch_device2), then the analytic partials of the Rayleigh ellipticity (K5 in surfdisp_kernels.hip).
int surfdisp_forward_ellip_kernels_device(void *stream, int B, int Lmax, const int *nlay,
                                          const float *model, int P, const float *per, int kind,
                                          float *c, float *u, float *ratio, int *status,
                                          float *dcdb, float *dcda, float *dcdr,
                                          float *dedb, float *deda, float *dedr, int *n_nonfinite,
                                          void *workspace, size_t workspace_bytes)
{
    int rc = entry_preamble("surfdisp_forward_ellip_kernels_device", ratio && dedb && dcdb, "ratio, dedb or dcdb",
                            SURFDISP_PHASE_ONLY | SURFDISP_KERN_REFCOORD | SURFDISP_STRICT, "no PHASE_ONLY, no KERN_REFCOORD, no STRICT",
                            (kind & ~SD_KIND_FLAGS) == SURFDISP_KIND_RAYLEIGH ? nullptr : "Rayleigh only (Love waves have no ellipticity)",
                            B, Lmax, P, kind, model, per, c, u, workspace, workspace_bytes, WS_ELLIP,
                            "surfdisp_ellip_kernels_workspace_bytes", SURFDISP_ERR_INVALID);
    if (rc) return rc;
    ForwardOpts o;
    o.dcdb = dcdb; o.dcda = dcda; o.dcdr = dcdr;
    o.ratio = ratio; o.record_history = true;
    rc = forward_device_impl(stream, B, Lmax, nlay, model, P, per, kind, c, u, status, workspace, workspace_bytes, o);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Layout lay = layout(workspace, B, Lmax, P, WS_ELLIP);
    const Carve &w = lay.w;
    const ECarve &e = lay.e;
    if (n_nonfinite) SD_HIP(hipMemsetAsync(n_nonfinite, 0, sizeof(int), s));
    sd::EllipKernArgs ea{B, Lmax, P, w.mdl, w.nl, per, w.ct, w.hist, w.nsolved, e.kpk, e.wscr, e.xscr, e.fscr, e.gam, e.khs,
                         n_nonfinite};
    sd::EllipTransposeArgs ta{B, P, Lmax, e.xscr, e.fscr, e.gam, e.khs, dedb, deda, dedr};
    SD_HIP(sd::launch_ellip_kern(s, ea, ta));
    return SURFDISP_SUCCESS;
}

// The same launches as surfdisp_forward_kernels_device (c, u, status, dc* bit for bit), then the apparent attenuation of the
// mode from the layer-major scratch those launches leave (K2c in surfdisp_kernels.hip).  Workspace: the kernels entry's.
int surfdisp_forward_atten_device(void *stream, int B, int Lmax, const int *nlay,
                                  const float *model, int P, const float *per, int kind,
                                  float *c, float *u, int *status,
                                  float *dcdb, float *dcda, float *dcdr,
                                  float *qinv, float *gamma, float *dqdq,
                                  void *workspace, size_t workspace_bytes)
{
    int rc = entry_preamble("surfdisp_forward_atten_device", qinv && dcdb, "qinv or dcdb",
                            SURFDISP_PHASE_ONLY | SURFDISP_KERN_REFCOORD, "no PHASE_ONLY, no KERN_REFCOORD", nullptr,
                            B, Lmax, P, kind, model, per, c, u, workspace, workspace_bytes, WS_KERNELS,
                            "surfdisp_atten_workspace_bytes", SURFDISP_ERR_INVALID);
    if (rc) return rc;
    ForwardOpts o;
    o.dcdb = dcdb; o.dcda = dcda; o.dcdr = dcdr;
    o.keep_vp_plane = true;
    rc = forward_device_impl(stream, B, Lmax, nlay, model, P, per, kind, c, u, status, workspace, workspace_bytes, o);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int wave = kind & ~SD_KIND_FLAGS;
    const Layout lay = layout(workspace, B, Lmax, P, WS_KERNELS);
    const Carve &w = lay.w;
    const KCarve &k = lay.k;                                                    // forward_device_impl's scratch, factors, layers
    sd::AttenArgs aa{B, P, Lmax, wave, w.mdl, per, k.kscr, k.kscale, k.khs, w.ct, w.ut, qinv, gamma, dqdq};
    SD_HIP(sd::launch_atten(s, aa));
    return SURFDISP_SUCCESS;
}

// The launches of surfdisp_forward_batch_device with the group-velocity kernel's EIG instantiation in place of the plain one
// (c, u, status bit for bit), then the transposition of the layer-top eigenfunctions and the energy integrals (K2d in
// surfdisp_kernels.hip).  Workspace: the forward solve's + the eigen region; no direct route.
int surfdisp_forward_eigen_device(void *stream, int B, int Lmax, const int *nlay,
                                  const float *model, int P, const float *per, int kind,
                                  float *c, float *u, int *status,
                                  float *ur, float *uz, float *tz, float *tr, float *energy,
                                  void *workspace, size_t workspace_bytes)
{
    int rc = entry_preamble("surfdisp_forward_eigen_device", c && u && status && ur, "c, u, status or ur",
                            SURFDISP_PHASE_ONLY | SURFDISP_KERN_REFCOORD, "no PHASE_ONLY, no KERN_REFCOORD", nullptr,
                            B, Lmax, P, kind, model, per, c, u, workspace, workspace_bytes, WS_EIGEN,
                            "surfdisp_eigen_workspace_bytes", SURFDISP_ERR_INVALID);
    if (rc) return rc;
    const Layout lay = layout(workspace, B, Lmax, P, WS_EIGEN);
    const Carve &w = lay.w;
    const EigCarve &e = lay.eig;
    ForwardOpts o;
    o.eigen = &e;
    rc = forward_device_impl(stream, B, Lmax, nlay, model, P, per, kind, c, u, status, workspace, workspace_bytes, o);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int wave = kind & ~SD_KIND_FLAGS;
    sd::EigenTransposeArgs ta{B, P, Lmax, wave, w.mdl, w.nl, per, e.escr, e.ediv, e.ehs, e.esum, w.ct, w.ut, ur, uz, tz, tr, energy};
    SD_HIP(sd::launch_eigen_transpose(s, ta));
    return SURFDISP_SUCCESS;
}

// The same launches as surfdisp_forward_kernels_device (c, u, status, dc* bit for bit), then the EIG instantiation of the
// group-velocity kernel on the roots and ellipticities those launches left (no second root search; its U goes to a scratch
// plane), then the thickness kernel on both layer-major scratches (K2e in surfdisp_kernels.hip).  Workspace: the kernels
// entry's, then the eigen region, then the scratch plane; no direct route.
int surfdisp_forward_thickness_kernels_device(void *stream, int B, int Lmax, const int *nlay,
                                              const float *model, int P, const float *per, int kind,
                                              float *c, float *u, int *status,
                                              float *dcdb, float *dcda, float *dcdr,
                                              float *dcdh, float *dcdz, int *n_nonfinite,
                                              void *workspace, size_t workspace_bytes)
{
    int rc = entry_preamble("surfdisp_forward_thickness_kernels_device", c && u && status && dcdb && dcdh,
                            "c, u, status, dcdb or dcdh", SURFDISP_PHASE_ONLY | SURFDISP_KERN_REFCOORD,
                            "no PHASE_ONLY, no KERN_REFCOORD", nullptr, B, Lmax, P, kind, model, per, c, u, workspace, workspace_bytes,
                            WS_THICK, "surfdisp_thickness_kernels_workspace_bytes", SURFDISP_ERR_INVALID);
    if (rc) return rc;
    ForwardOpts o;
    o.dcdb = dcdb; o.dcda = dcda; o.dcdr = dcdr;
    o.keep_vp_plane = o.keep_rho_plane = true;
    rc = forward_device_impl(stream, B, Lmax, nlay, model, P, per, kind, c, u, status, workspace, workspace_bytes, o);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int wave = kind & ~SD_KIND_FLAGS;
    const Layout lay = layout(workspace, B, Lmax, P, WS_THICK);
    const Carve &w = lay.w;
    const KCarve &k = lay.k;                                                    // forward_device_impl's scratch, factors, layers
    if (n_nonfinite) SD_HIP(hipMemsetAsync(n_nonfinite, 0, sizeof(int), s));
    return thickness_pass(s, B, Lmax, P, wave, model, lay, per, w.ct, w.ratio, w.ut, k.kscr, k.kscale, k.khs, dcdh, dcdz, n_nonfinite);
}

// The launches of surfdisp_forward_group_kernels_device and of surfdisp_forward_thickness_kernels_device in one pass (c .. dcdr,
// dudb .. dudr, dcdh, dcdz bit for bit), and the thickness kernel again at the two shifted periods: dU/d(layer thickness, interface
// depth) by the rule of K4 (K4d in surfdisp_group_thick.hip).  Workspace: the group entry's, then the eigen region, the U plane and
// the four row planes; no direct route.
int surfdisp_forward_group_thickness_kernels_device(void *stream, int B, int Lmax, const int *nlay,
                                                    const float *model, int P, const float *per, int kind, float dlnT_frac,
                                                    float *c, float *u, int *status,
                                                    float *dcdb, float *dcda, float *dcdr,
                                                    float *dudb, float *duda, float *dudr,
                                                    float *dcdh, float *dcdz, float *dudh, float *dudz,
                                                    int *n_shift_failed, int *n_nonfinite,
                                                    void *workspace, size_t workspace_bytes)
{
    int rc = entry_preamble("surfdisp_forward_group_thickness_kernels_device", c && u && status && dcdb && dudb && dcdh && dudh,
                            "c, u, status, dcdb, dudb, dcdh or dudh", SURFDISP_PHASE_ONLY | SURFDISP_KERN_REFCOORD,
                            "no PHASE_ONLY, no KERN_REFCOORD",
                            (dlnT_frac >= 1.0e-3f && dlnT_frac <= 0.05f) ? nullptr : "dlnT_frac outside [1e-3, 0.05]",
                            B, Lmax, P, kind, model, per, c, u, workspace, workspace_bytes, WS_GROUP_THICK,
                            "surfdisp_group_thickness_kernels_workspace_size", SURFDISP_ERR_INVALID);
    if (rc) return rc;
    const GroupThickOuts t{dcdh, dcdz, dudh, dudz, n_nonfinite};
    return group_launches(stream, B, Lmax, nlay, model, P, per, kind, dlnT_frac, c, u, status, dcdb, dcda, dcdr, dudb, duda, dudr,
                          n_shift_failed, workspace, workspace_bytes, WS_GROUP_THICK, &t);
}

// Parameters -> layer stacks on the device for a static-structure model; the
// descriptor layout is documented in surfdisp_layers.hip and built by pysurfinv_amd.layers_batch.
int surfdisp_params_to_model_device(void *stream, int C, int N, int L, const double *params,
                                    const int *idesc, const double *fdesc, float *model)
{
    if (C < 1 || N < 0 || L < 2 || L > SURFDISP_NLAY_MAX || !params || !idesc || !fdesc || !model) {
        set_err("surfdisp_params_to_model_device: bad argument");
        return SURFDISP_ERR_INVALID;
    }
    sd::LayersArgs a{C, N, params, idesc, fdesc, model, nullptr};
    SD_HIP(sd::launch_layers(static_cast<hipStream_t>(stream), a, L));
    return SURFDISP_SUCCESS;
}

// Same for a model with one thermal mantle layer (OceanMantleHybrid): the thermal
// kernel fills scratch ([C][64][2] doubles, caller-owned: no allocation, graph-capturable), the layer
// kernel assembles the stack.
size_t surfdisp_thermal_scratch_bytes(int C)
{
    return C < 1 ? 0 : (size_t)C * 64 * 2 * sizeof(double);
}

int surfdisp_params_to_model_thermal_device(void *stream, int C, int N, int L, const double *params,
                                            const int *idesc, const double *fdesc,
                                            void *scratch, size_t scratch_bytes, float *model)
{
    if (C < 1 || N < 0 || L < 2 || L > SURFDISP_NLAY_MAX || !params || !idesc || !fdesc || !model || !scratch) {
        set_err("surfdisp_params_to_model_thermal_device: bad argument");
        return SURFDISP_ERR_INVALID;
    }
    if (scratch_bytes < surfdisp_thermal_scratch_bytes(C)) {
        set_err("surfdisp_params_to_model_thermal_device: scratch too small (surfdisp_thermal_scratch_bytes)");
        return SURFDISP_ERR_INVALID;
    }
    sd::LayersArgs a{C, N, params, idesc, fdesc, model, static_cast<double *>(scratch)};
    SD_HIP(sd::launch_thermal(static_cast<hipStream_t>(stream), a));
    SD_HIP(sd::launch_layers(static_cast<hipStream_t>(stream), a, L));
    return SURFDISP_SUCCESS;
}

// Metropolis glue on the device (surfdisp_mcmc.hip): proposal and misfit / accept / state update of one lock step.
// The three proposal entries: one proposal per chain (depth 1), the speculative tree (depth > 1), or the masked redraw (tags).
static int mcmc_propose(const char *name, void *stream, int C, int N, const double *p, const double *vmin, const double *vmax,
                        const double *step, unsigned long long seed, unsigned long long counter, int reset, double *out, long chain0,
                        int depth, bool masked, const unsigned char *tags, int attempt, int tag)
{
    if (C < 1 || N < 1 || !p || !vmin || !vmax || !step || !out || chain0 < 0 || depth < 1 || depth > sd::SD_MCMC_MAX_DEPTH ||
        (masked && (!tags || attempt < 0 || attempt > 1023 || reset < 0 || reset > 2 || tag < 1 || tag > 255))) {
        set_err("%s: bad argument%s", name, depth != 1 ? " (1 <= depth <= 4)" : ""); return SURFDISP_ERR_INVALID;
    }
    sd::McmcProposeArgs a{C, N, p, vmin, vmax, step, seed, counter, reset, out, chain0, depth, tags, attempt, tag};
    SD_HIP(sd::launch_mcmc_propose(static_cast<hipStream_t>(stream), a));
    return SURFDISP_SUCCESS;
}

int surfdisp_mcmc_propose_device(void *stream, int C, int N, const double *p, const double *vmin, const double *vmax,
                                 const double *step, unsigned long long seed, unsigned long long counter, int reset, double *out, long chain0)
{
    return mcmc_propose("surfdisp_mcmc_propose_device", stream, C, N, p, vmin, vmax, step, seed, counter, reset ? 1 : 0, out, chain0, 1,
                        false, nullptr, 0, 0);
}

// masked redraw of the chains the prior kernel tagged (tags[c] == tag; see surfdisp_prior_device); mode 0: bounded Gaussian step,
// 1: uniform prior draw, 2: the chain's state itself
int surfdisp_mcmc_propose_masked_device(void *stream, int C, int N, const double *p, const double *vmin, const double *vmax,
                                        const double *step, unsigned long long seed, unsigned long long counter, int attempt, int mode,
                                        const unsigned char *tags, int tag, double *out, long chain0)
{
    return mcmc_propose("surfdisp_mcmc_propose_masked_device", stream, C, N, p, vmin, vmax, step, seed, counter, mode, out, chain0, 1,
                        true, tags, attempt, tag);
}

int surfdisp_mcmc_propose_tree_device(void *stream, int C, int N, int depth, const double *p, const double *vmin, const double *vmax,
                                      const double *step, unsigned long long seed, unsigned long long counter, double *out, long chain0)
{
    return mcmc_propose("surfdisp_mcmc_propose_tree_device", stream, C, N, p, vmin, vmax, step, seed, counter, 0, out, chain0, depth,
                        false, nullptr, 0, 0);
}

// The proposal tree of a sampler with a prior, redrawn inside the kernel until the rules hold (csrc/surfdisp_mcmc_prior.hip; header
// section (6c)).  Every argument is judged on the host before anything touches the device.
int surfdisp_mcmc_propose_prior_device(void *stream, int C, int N, int K, int L, int depth,
                                       const double *p, const double *aux, const double *vmin, const double *vmax, const double *step,
                                       const int *idesc, const double *fdesc, const int *flags, double vs_max,
                                       int gauss_tries, int uniform_tries,
                                       unsigned long long seed, unsigned long long counter, long chain0,
                                       double *out, unsigned short *tries, int *exhausted)
{
    const char *name = "surfdisp_mcmc_propose_prior_device";
    if (C < 1 || N < 1 || K < 0 || L < 1 || L > SURFDISP_NLAY_MAX || depth < 1 || depth > sd::SD_MCMC_MAX_DEPTH) {
        set_err("%s: invalid size (C >= 1; N >= 1; K >= 0; 1 <= L <= SURFDISP_NLAY_MAX; 1 <= depth <= 4)", name);
        return SURFDISP_ERR_INVALID;
    }
    if ((long)N + (long)K > sd::SD_MCMC_PRIOR_ROW) {
        set_err("%s: invalid size: N + K beyond the SURFDISP_MCMC_PRIOR_ROW_MAX = 256 doubles of the row in LDS", name);
        return SURFDISP_ERR_INVALID;
    }
    if (gauss_tries < 0 || uniform_tries < 0 || (long)gauss_tries + uniform_tries < 1 ||
        (long)gauss_tries + uniform_tries > sd::SD_MCMC_PRIOR_TRIES) {
        set_err("%s: invalid caps: gauss_tries >= 0, uniform_tries >= 0, 1 <= their sum <= 16384", name);
        return SURFDISP_ERR_INVALID;
    }
    // (chain0 + C) * N < 2^48: the retry index sits above bit 48 of the stream index
    const long lim = 1L << 48;
    if (chain0 < 0 || chain0 >= lim || chain0 + (long)C > (lim - 1) / N) {
        set_err("%s: invalid chain0: (chain0 + C) * N must stay below 2^48", name); return SURFDISP_ERR_INVALID;
    }
    if (!p || !vmin || !vmax || !step || !idesc || !fdesc || !flags || !out || !exhausted || (K > 0 && !aux)) {
        set_err("%s: invalid argument: a required pointer is NULL", name); return SURFDISP_ERR_INVALID;
    }
    sd::McmcPriorArgs a{C, N, K, L, depth, p, aux, vmin, vmax, step, idesc, fdesc, flags, vs_max, gauss_tries, uniform_tries,
                        seed, counter, chain0, out, tries, exhausted};
    SD_HIP(sd::launch_mcmc_propose_prior(static_cast<hipStream_t>(stream), a));
    return SURFDISP_SUCCESS;
}

// The same tree with proposals shaped by a per-point factor, and the factor from a covariance (csrc/surfdisp_mcmc_cov.hip; header
// section (6c)).  Every argument is judged on the host before anything touches the device.
int surfdisp_mcmc_propose_cov_device(void *stream, int C, int N, int K, int L, int depth,
                                     const double *p, const double *aux, const double *vmin, const double *vmax,
                                     const double *factor_t, long chains_per_factor, int F,
                                     const int *idesc, const double *fdesc, const int *flags, double vs_max,
                                     int gauss_tries, int uniform_tries,
                                     unsigned long long seed, unsigned long long counter, long chain0,
                                     double *out, unsigned short *tries, int *exhausted)
{
    const char *name = "surfdisp_mcmc_propose_cov_device";
    if (C < 1 || N < 1 || N > sd::SD_MCMC_COV_MAX_N || K < 0 || depth < 1 || depth > sd::SD_MCMC_MAX_DEPTH) {
        set_err("%s: invalid size (C >= 1; 1 <= N <= SURFDISP_MCMC_COV_N_MAX = 64; K >= 0; 1 <= depth <= 4)", name);
        return SURFDISP_ERR_INVALID;
    }
    if (flags) {
        if (L < 1 || L > SURFDISP_NLAY_MAX || (long)N + (long)K > sd::SD_MCMC_PRIOR_ROW) {
            set_err("%s: invalid size with flags (1 <= L <= SURFDISP_NLAY_MAX; N + K <= SURFDISP_MCMC_PRIOR_ROW_MAX = 256)", name);
            return SURFDISP_ERR_INVALID;
        }
        if (!idesc || !fdesc || (K > 0 && !aux)) {
            set_err("%s: invalid argument: flags without idesc / fdesc (or K > 0 without aux)", name); return SURFDISP_ERR_INVALID;
        }
    } else if (idesc || fdesc || aux || K != 0 || L != 0) {
        set_err("%s: invalid argument: without flags there are no rules: idesc, fdesc and aux NULL, K = L = 0", name);
        return SURFDISP_ERR_INVALID;
    }
    if (gauss_tries < 0 || uniform_tries < 0 || (long)gauss_tries + uniform_tries < 1 ||
        (long)gauss_tries + uniform_tries > sd::SD_MCMC_PRIOR_TRIES) {
        set_err("%s: invalid caps: gauss_tries >= 0, uniform_tries >= 0, 1 <= their sum <= 16384", name);
        return SURFDISP_ERR_INVALID;
    }
    // (chain0 + C) * N < 2^48: the retry index sits above bit 48 of the stream index
    const long lim = 1L << 48;
    if (chain0 < 0 || chain0 >= lim || chain0 + (long)C > (lim - 1) / N) {
        set_err("%s: invalid chain0: (chain0 + C) * N must stay below 2^48", name); return SURFDISP_ERR_INVALID;
    }
    if (chains_per_factor < 1 || F < 1 || (chain0 + (long)C - 1) / chains_per_factor >= (long)F) {
        set_err("%s: invalid factor index: chains_per_factor >= 1, F >= 1, (chain0 + C - 1) / chains_per_factor < F", name);
        return SURFDISP_ERR_INVALID;
    }
    if (!p || !vmin || !vmax || !factor_t || !out || !exhausted) {
        set_err("%s: invalid argument: a required pointer is NULL", name); return SURFDISP_ERR_INVALID;
    }
    sd::McmcCovArgs a{C, N, K, L, depth, p, aux, vmin, vmax, factor_t, chains_per_factor, idesc, fdesc, flags, vs_max,
                      gauss_tries, uniform_tries, seed, counter, chain0, out, tries, exhausted};
    SD_HIP(sd::launch_mcmc_propose_cov(static_cast<hipStream_t>(stream), a));
    return SURFDISP_SUCCESS;
}

int surfdisp_mcmc_cov_factor_device(void *stream, int P, int N, const double *cov, double scale, const double *fallback_step,
                                    double *factor_t, int *flag)
{
    const char *name = "surfdisp_mcmc_cov_factor_device";
    if (P < 1 || N < 1 || N > sd::SD_MCMC_COV_MAX_N) {
        set_err("%s: invalid size (P >= 1; 1 <= N <= SURFDISP_MCMC_COV_N_MAX = 64)", name); return SURFDISP_ERR_INVALID;
    }
    if (!cov || !fallback_step || !factor_t || !flag) {
        set_err("%s: invalid argument: a required pointer is NULL", name); return SURFDISP_ERR_INVALID;
    }
    sd::McmcCovFactorArgs a{P, N, cov, scale, fallback_step, factor_t, flag};
    SD_HIP(sd::launch_mcmc_cov_factor(static_cast<hipStream_t>(stream), a));
    return SURFDISP_SUCCESS;
}

// One pooled adaptive-Metropolis update per point (csrc/surfdisp_mcmc_adapt.hip; header section (6c)).  Every argument is judged on
// the host before anything touches the device; the comparisons are written so that a NaN fails them.
int surfdisp_mcmc_adapt_device(void *stream, int F, int cpp, int N, const double *p,
                               const double *track, long chain_stride, long row_stride, int row_lo, int row_hi,
                               const double *step, double forget, double target_accept, double gain, double decay,
                               double ls_min, double ls_max, double min_weight, double ridge,
                               double *state, double *cov_out)
{
    const char *name = "surfdisp_mcmc_adapt_device";
    if (F < 1 || cpp < 1 || N < 1 || N > sd::SD_MCMC_COV_MAX_N) {
        set_err("%s: invalid size (F >= 1; cpp >= 1; 1 <= N <= SURFDISP_MCMC_COV_N_MAX = 64)", name); return SURFDISP_ERR_INVALID;
    }
    if (!(forget > 0.0 && forget <= 1.0)) {
        set_err("%s: invalid forget: 0 < forget <= 1 expected", name); return SURFDISP_ERR_INVALID;
    }
    if (row_lo < 0 || row_hi < row_lo) {
        set_err("%s: invalid window: 0 <= row_lo <= row_hi expected", name); return SURFDISP_ERR_INVALID;
    }
    if (!(ridge >= 0.0) || !(min_weight >= 1.0) || !(ls_min <= ls_max) || !(target_accept <= 1.0) || !(gain == gain) || !(decay == decay)) {
        set_err("%s: invalid option: ridge >= 0, min_weight >= 1, ls_min <= ls_max, target_accept <= 1 and numbers for gain and decay expected",
                name);
        return SURFDISP_ERR_INVALID;
    }
    if (!p || !state || !step || (!track && target_accept >= 0.0 && row_hi > row_lo)) {
        set_err("%s: invalid argument: a required pointer is NULL (p, state, step; track with a window to read)", name);
        return SURFDISP_ERR_INVALID;
    }
    sd::McmcAdaptArgs a{F, cpp, N, p, track, chain_stride, row_stride, row_lo, row_hi, step, forget, target_accept, gain, decay,
                        ls_min, ls_max, min_weight, ridge, state, cov_out};
    SD_HIP(sd::launch_mcmc_adapt(static_cast<hipStream_t>(stream), a));
    return SURFDISP_SUCCESS;
}

// Posterior Vs(z) profiles of a Metropolis track (csrc/surfdisp_post.hip; header section (6f)).  Workspace: the per-slab partials
// [npoints][nslab][D + N][5] doubles, the slabs' smallest misfits [npoints][nslab] doubles, then four int arrays [npoints][nslab].
static long post_slabs(int R) { return ((long)R + SURFDISP_POST_SLAB_ROWS - 1) / SURFDISP_POST_SLAB_ROWS; }

size_t surfdisp_posterior_workspace_bytes(int npoints, int R, int N, int D)
{
    if (npoints < 1 || R < 1 || N < 1 || D < 1) return 0;
    const size_t units = (size_t)npoints * (size_t)post_slabs(R);
    return units * ((size_t)(D + N) * 5 * sizeof(double) + sizeof(double) + 4 * sizeof(int));
}

// What the two entries on a track ((6f) profiles, (6g) sources) share: the sizes both refuse (each with its own text), ...
static bool post_track_sizes_ok(int npoints, int R, long row_stride, long min_stride)
{
    return npoints >= 1 && R >= 1 && R <= (1 << 30) && row_stride >= min_stride && (long)npoints * post_slabs(R) <= 0x7fffffffL;
}
// ... the prefix rule, ...
static int post_check_prefix(const char *name, int R, int chainL, int prefix)
{
    if (chainL > 0 && (prefix < 1 || prefix > chainL || R % chainL != 0)) {
        set_err("%s: invalid prefix: 1 <= prefix <= chainL and R a multiple of chainL", name); return SURFDISP_ERR_INVALID;
    }
    return SURFDISP_SUCCESS;
}

// ... and the selection part of a PostArgs (what launch_post_selection reads and writes): sizes, rule, track, the four selection
// outputs and the [npoints][nslab] tail of the workspace from `tail` on - doubles first, then the four int arrays.
static void post_fill_selection(sd::PostArgs &a, int npoints, int R, const double *track, long row_stride, int true_markov_chain,
                                int chainL, int prefix, double *min_misfit, double *thres, int *imin, int *n_final, void *tail)
{
    a.npoints = npoints; a.R = R; a.nslab = (int)post_slabs(R);
    a.tmc = true_markov_chain ? 1 : 0; a.chainL = chainL > 0 ? chainL : 0; a.prefix = prefix;
    a.row_stride = row_stride; a.track = track;
    a.min_misfit = min_misfit; a.thres = thres; a.imin = imin; a.n_final = n_final;
    const size_t units = (size_t)npoints * a.nslab;
    a.ws_mis = static_cast<double *>(tail);
    a.ws_row = reinterpret_cast<int *>(a.ws_mis + units);
    a.ws_last = a.ws_row + units; a.ws_carry = a.ws_last + units; a.ws_nfin = a.ws_carry + units;
}

// hist [cols][nbins], below [cols], above [cols] zeroed on the stream: the kernels add into them
static int post_zero_hist(hipStream_t s, int *hist, int *below, int *above, size_t cols, int nbins)
{
    SD_HIP(hipMemsetAsync(hist, 0, cols * nbins * sizeof(int), s));
    SD_HIP(hipMemsetAsync(below, 0, cols * sizeof(int), s));
    SD_HIP(hipMemsetAsync(above, 0, cols * sizeof(int), s));
    return SURFDISP_SUCCESS;
}

// the integer part of the params->stack descriptor (layout: csrc/surfdisp_layers.hip), as the profile kernel walks it
static const char *post_check_desc(const int *idesc, int len, int width, bool has_aux, int N)
{
    if (len < 4) return "descriptor too short";
    const int nin = idesc[0], ngrid = idesc[1];
    if (nin < 1 || nin > sd::SD_POST_MAX_LAYERS) return "1..10 input layers";
    if (len < 4 + 16 * nin) return "descriptor too short";
    auto slot_ok = [&](int sl) { return sl >= -1 && sl < width && (has_aux || sl < N); };
    int at = 0;
    for (int l = 0; l < nin; ++l) {
        const int *li = idesc + 4 + 8 * l, *ci = idesc + 4 + 8 * nin + 8 * l;
        if (li[0] == 6) return "a thermal layer (kind 6) is not supported";
        if (li[0] < 0 || li[0] > 7) return "unknown layer kind";
        if (!slot_ok(li[1]) || li[3] < 0 || li[3] > 8) return "thickness slot or coefficient count out of range";
        if (li[4] != at || li[5] < li[4] + 2) return "grid ranges must tile 0..ngrid in order, two points or more each";
        at = li[5];
        for (int k = 0; k < li[3]; ++k)
            if (!slot_ok(ci[k])) return "coefficient slot out of range";
    }
    if (at != ngrid) return "grid ranges must tile 0..ngrid in order, two points or more each";
    if (idesc[4 + 6] < 0 || !slot_ok(idesc[4 + 6] - 1)) return "topography slot out of range";
    return nullptr;
}

int surfdisp_posterior_profile_device(void *stream, int npoints, int R, int N, const double *track, long row_stride,
                                      const int *idesc, int idesc_len, const double *fdesc,
                                      const double *aux, int K, const int *rows,
                                      int D, const double *zdeps, int true_markov_chain, int chainL, int prefix,
                                      int nbins, double vlo, double vhi,
                                      double *min_misfit, double *thres, int *imin, int *n_final,
                                      double *pmean, double *pstd,
                                      int *count, double *vs_mean, double *vs_std, double *vs_min, double *vs_max,
                                      int *hist, int *below, int *above,
                                      void *workspace, size_t workspace_bytes)
{
    const char *name = "surfdisp_posterior_profile_device";
    if (!post_track_sizes_ok(npoints, R, row_stride, 3 + (long)N) || N < 1 || N > sd::SD_POST_MAX_PARAMS || K < 0 || D < 1 ||
        D > SURFDISP_POST_DEPTHS_MAX) {
        set_err("%s: invalid size (npoints, R, N >= 1; N <= 128; R <= 2^30; row_stride >= 3 + N; K >= 0; 1 <= D <= 256)", name);
        return SURFDISP_ERR_INVALID;
    }
    if (!track || !idesc || !fdesc || !zdeps || !min_misfit || !thres || !imin || !n_final || !count || !vs_mean || !vs_std ||
        !vs_min || !vs_max || !workspace || (!pmean != !pstd) || (hist && (!below || !above)) || (K > 0 && !aux)) {
        set_err("%s: invalid argument: a required pointer is NULL", name); return SURFDISP_ERR_INVALID;
    }
    for (int d = 0; d < D; ++d)
        if (!std::isfinite(zdeps[d]) || (d > 0 && !(zdeps[d] > zdeps[d - 1]))) {
            set_err("%s: invalid depths: finite and strictly ascending", name); return SURFDISP_ERR_INVALID;
        }
    if (hist && (nbins < 1 || !std::isfinite(vlo) || !std::isfinite(vhi) || !(vhi > vlo))) {
        set_err("%s: invalid histogram: nbins >= 1, finite vlo < vhi", name); return SURFDISP_ERR_INVALID;
    }
    if (int rc = post_check_prefix(name, R, chainL, prefix)) return rc;
    if (const char *why = post_check_desc(idesc, idesc_len, N + K, aux != nullptr, N)) {
        set_err("%s: invalid descriptor: %s", name, why); return SURFDISP_ERR_INVALID;
    }
    if (workspace_bytes < surfdisp_posterior_workspace_bytes(npoints, R, N, D)) {
        set_err("%s: invalid workspace: smaller than surfdisp_posterior_workspace_bytes", name); return SURFDISP_ERR_INVALID;
    }
    sd::PostArgs a{};
    a.ws_part = static_cast<double *>(workspace);
    post_fill_selection(a, npoints, R, track, row_stride, true_markov_chain, chainL, prefix, min_misfit, thres, imin, n_final,
                        a.ws_part + (size_t)npoints * (size_t)post_slabs(R) * (size_t)(D + N) * 5);
    a.N = N; a.K = K; a.D = D; a.fdesc = fdesc; a.aux = aux; a.rows = aux ? rows : nullptr; a.pmean = pmean; a.pstd = pstd;
    a.count = count; a.vs_mean = vs_mean; a.vs_std = vs_std; a.vs_min = vs_min; a.vs_max = vs_max;
    const int nin = idesc[0];
    for (int i = 0; i < 4 + 16 * nin; ++i) a.idesc[i] = idesc[i];
    for (int d = 0; d < D; ++d) a.zdeps[d] = zdeps[d];
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hist) {
        a.hist = hist; a.below = below; a.above = above; a.nbins = nbins; a.vlo = vlo; a.vhi = vhi;
        a.bin_w = (vhi - vlo) / nbins; a.inv_w = nbins / (vhi - vlo);
        if (int rc = post_zero_hist(s, hist, below, above, (size_t)npoints * D, nbins)) return rc;
    }
    SD_HIP(sd::launch_posterior(s, a));
    return SURFDISP_SUCCESS;
}

// Source rows of a Metropolis track (csrc/surfdisp_pred.hip; header section (6g)).  Workspace: the slabs' smallest misfits
// [npoints][nslab] doubles, then four int arrays [npoints][nslab] (as the tail of the (6f) workspace).
size_t surfdisp_posterior_sources_workspace_bytes(int npoints, int R)
{
    if (npoints < 1 || R < 1) return 0;
    return (size_t)npoints * (size_t)post_slabs(R) * (sizeof(double) + 4 * sizeof(int));
}

int surfdisp_posterior_sources_device(void *stream, int npoints, int R, const double *track, long row_stride,
                                      int true_markov_chain, int chainL, int prefix,
                                      double *min_misfit, double *thres, int *imin, int *n_final,
                                      int *weight, int *n_sources, int *imin_source,
                                      void *workspace, size_t workspace_bytes)
{
    const char *name = "surfdisp_posterior_sources_device";
    if (!post_track_sizes_ok(npoints, R, row_stride, 3)) {
        set_err("%s: invalid size (npoints, R >= 1; R <= 2^30; row_stride >= 3; npoints x slabs <= 2^31 - 1)", name);
        return SURFDISP_ERR_INVALID;
    }
    if (!track || !min_misfit || !thres || !imin || !n_final || !weight || !n_sources || !imin_source || !workspace) {
        set_err("%s: invalid argument: a required pointer is NULL", name); return SURFDISP_ERR_INVALID;
    }
    if (int rc = post_check_prefix(name, R, chainL, prefix)) return rc;
    if (workspace_bytes < surfdisp_posterior_sources_workspace_bytes(npoints, R)) {
        set_err("%s: invalid workspace: smaller than surfdisp_posterior_sources_workspace_bytes", name); return SURFDISP_ERR_INVALID;
    }
    sd::PostSourcesArgs S{};
    post_fill_selection(S.sel, npoints, R, track, row_stride, true_markov_chain, chainL, prefix, min_misfit, thres, imin, n_final,
                        workspace);
    S.weight = weight; S.n_sources = n_sources; S.imin_source = imin_source;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SD_HIP(hipMemsetAsync(weight, 0, (size_t)npoints * R * sizeof(int), s));
    SD_HIP(sd::launch_post_sources(s, S));
    return SURFDISP_SUCCESS;
}

// Weighted column statistics of a list of predictions (csrc/surfdisp_pred.hip; header section (6g)).  Workspace: the partials
// [npoints][nslab][P][5] doubles, then the slabs' failed weights [npoints][nslab] ints.
static long pred_slabs(long total)
{
    const long n = (total + SURFDISP_PRED_SLAB_ROWS - 1) / SURFDISP_PRED_SLAB_ROWS;
    return n < 1 ? 1 : (n > SURFDISP_PRED_SLABS_MAX ? SURFDISP_PRED_SLABS_MAX : n);
}

size_t surfdisp_posterior_predictive_workspace_bytes(int npoints, int total, int P)
{
    if (npoints < 1 || total < 0 || P < 1) return 0;
    const size_t units = (size_t)npoints * (size_t)pred_slabs(total);
    return units * ((size_t)P * 5 * sizeof(double) + sizeof(int));
}

int surfdisp_posterior_predictive_device(void *stream, int npoints, int total, int P, const float *pred, long ld,
                                         const unsigned char *failed, const int *w, const int *offsets,
                                         int nbins, const double *vlo, const double *vhi,
                                         int *count, double *mean, double *std, double *vmin, double *vmax, int *n_failed,
                                         int *hist, int *below, int *above,
                                         void *workspace, size_t workspace_bytes)
{
    const char *name = "surfdisp_posterior_predictive_device";
    if (npoints < 1 || total < 0 || P < 1 || P > SURFDISP_PRED_COLS_MAX || ld < (long)P ||
        (long)npoints * pred_slabs(total) > 0x7fffffffL) {
        set_err("%s: invalid size (npoints >= 1; total >= 0; 1 <= P <= 1024; ld >= P; npoints x slabs <= 2^31 - 1)", name);
        return SURFDISP_ERR_INVALID;
    }
    if ((total > 0 && (!pred || !w)) || !offsets || !count || !mean || !std || !vmin || !vmax || !n_failed || !workspace ||
        (hist && (!below || !above || !vlo || !vhi))) {
        set_err("%s: invalid argument: a required pointer is NULL", name); return SURFDISP_ERR_INVALID;
    }
    if (hist) {
        bool ok = nbins >= 1;
        for (int c = 0; ok && c < P; ++c) ok = std::isfinite(vlo[c]) && std::isfinite(vhi[c]) && vhi[c] > vlo[c];
        if (!ok) { set_err("%s: invalid histogram: nbins >= 1, finite vlo < vhi in every column", name); return SURFDISP_ERR_INVALID; }
    }
    if (workspace_bytes < surfdisp_posterior_predictive_workspace_bytes(npoints, total, P)) {
        set_err("%s: invalid workspace: smaller than surfdisp_posterior_predictive_workspace_bytes", name); return SURFDISP_ERR_INVALID;
    }
    sd::PredArgs a{};
    a.npoints = npoints; a.total = total; a.P = P; a.nslab = (int)pred_slabs(total); a.ld = ld;
    a.pred = pred; a.failed = failed; a.w = w; a.offsets = offsets;
    a.count = count; a.mean = mean; a.std = std; a.mn = vmin; a.mx = vmax; a.n_failed = n_failed;
    const size_t units = (size_t)npoints * a.nslab;
    a.ws_part = static_cast<double *>(workspace);
    a.ws_nfail = reinterpret_cast<int *>(a.ws_part + units * (size_t)P * 5);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hist) {
        a.hist = hist; a.below = below; a.above = above; a.nbins = nbins;
        if (int rc = post_zero_hist(s, hist, below, above, (size_t)npoints * P, nbins)) return rc;
    }
    SD_HIP(sd::launch_pred_stats(s, a, vlo, vhi));
    return SURFDISP_SUCCESS;
}

// The generic prior predicates on the device (csrc/surfdisp_layers.hip, surfdisp_prior_kernel): tags[c] = mark_tag where chain c's
// model breaks a rule; only_tag >= 0: only chains with tags[c] >= only_tag are looked at.  Static-structure models, no thermal layer.
int surfdisp_prior_device(void *stream, int C, int N, int L, const double *params, const int *idesc, const double *fdesc,
                          const int *flags, double vs_max, int only_tag, int mark_tag, unsigned char *tags)
{
    if (C < 1 || N < 0 || L < 1 || L > SURFDISP_NLAY_MAX || !params || !idesc || !fdesc || !flags || !tags || mark_tag < 1 || mark_tag > 255 ||
        only_tag >= mark_tag) {
        set_err("surfdisp_prior_device: bad argument"); return SURFDISP_ERR_INVALID;
    }
    sd::LayersArgs a{C, N, params, idesc, fdesc, nullptr, nullptr};
    SD_HIP(sd::launch_prior(static_cast<hipStream_t>(stream), a, L, flags, vs_max, only_tag, mark_tag, tags));
    return SURFDISP_SUCCESS;
}

// The two accept entries of the Rayleigh phase-velocity misfit.  need_chain0: surfdisp_mcmc_accept_tree_device rejects a negative
// chain0, surfdisp_mcmc_accept_device never did.
static int mcmc_accept(const char *name, bool need_chain0, void *stream, int C, int N, int P, const float *c, const int *status,
                       const double *c_obs, const double *uncer, const unsigned char *mask, int obs_per_chain,
                       const double *p1, double *p0, double *chi0, double *row, long row_stride, long step_stride,
                       unsigned long long seed, unsigned long long counter, int first, long chain0, int depth, int nsteps)
{
    if (C < 1 || N < 1 || P < 1 || depth < 1 || depth > sd::SD_MCMC_MAX_DEPTH || nsteps < 1 || nsteps > depth ||
        !c || !c_obs || !uncer || !mask || !p1 || !p0 || !chi0 || (need_chain0 && chain0 < 0)) {
        set_err("%s: bad argument%s", name, need_chain0 ? " (1 <= nsteps <= depth <= 4)" : ""); return SURFDISP_ERR_INVALID;
    }
    sd::McmcAcceptArgs a{C, N, P, c, status, c_obs, uncer, mask, obs_per_chain ? 1 : 0, p1, p0, chi0, row, row_stride, seed, counter,
                         first ? 1 : 0, chain0, depth, nsteps, step_stride};
    SD_HIP(sd::launch_mcmc_accept(static_cast<hipStream_t>(stream), a));
    return SURFDISP_SUCCESS;
}

int surfdisp_mcmc_accept_device(void *stream, int C, int N, int P, const float *c, const int *status,
                                const double *c_obs, const double *uncer, const unsigned char *mask, int obs_per_chain,
                                const double *p1, double *p0, double *chi0, double *row, long row_stride,
                                unsigned long long seed, unsigned long long counter, int first, long chain0)
{
    return mcmc_accept("surfdisp_mcmc_accept_device", false, stream, C, N, P, c, status, c_obs, uncer, mask, obs_per_chain, p1, p0, chi0,
                       row, row_stride, 0, seed, counter, first, chain0, 1, 1);
}

int surfdisp_mcmc_accept_tree_device(void *stream, int C, int N, int P, int depth, int nsteps, const float *c, const int *status,
                                     const double *c_obs, const double *uncer, const unsigned char *mask, int obs_per_chain,
                                     const double *q, double *p0, double *chi0, double *row, long row_stride, long step_stride,
                                     unsigned long long seed, unsigned long long counter, long chain0)
{
    return mcmc_accept("surfdisp_mcmc_accept_tree_device", true, stream, C, N, P, c, status, c_obs, uncer, mask, obs_per_chain, q, p0, chi0,
                       row, row_stride, step_stride, seed, counter, 0, chain0, depth, nsteps);
}

// Joint data (Rayleigh / Love, phase / group velocity): the accept entries above with the misfit summed over a column table.
// ellip: the five-array entries (pred[4] = the Rayleigh solve's ellipticity, NULL allowed; column sources 4 and 5).
static int mcmc_accept_joint(const char *name, bool ellip, void *stream, int C, int N, const float *const *pred, const long *pred_stride,
                             const int nper[2], const int *const status[2], int Ptot, const int *cols, const double *weights,
                             const double *obs, const double *uncer, const unsigned char *mask, int obs_per_chain,
                             const double *p1, double *p0, double *chi0, double *row, long row_stride, long step_stride,
                             unsigned long long seed, unsigned long long counter, int first, long chain0, int depth, int nsteps)
{
    bool ok = C >= 1 && N >= 1 && Ptot >= 1 && Ptot <= sd::SD_MCMC_JOINT_MAX_COLS && pred && pred_stride && nper && status && cols && weights && obs && uncer && mask &&
              p1 && p0 && chi0 && chain0 >= 0 && depth >= 1 && depth <= sd::SD_MCMC_MAX_DEPTH && nsteps >= 1 && nsteps <= depth;
    sd::McmcJointArgs j{};
    for (int w = 0; ok && w < 2; ++w) {
        j.nper[w] = nper[w];
        j.status[w] = status[w];
        if (!pred[2 * w] && pred[2 * w + 1]) ok = false;                  // a group array without the phase array of its solve
        for (int k = 2 * w; ok && k < 2 * w + 2; ++k) {
            j.pred[k] = pred[k];
            j.pstride[k] = pred_stride[k];
            if (pred[k] && (nper[w] < 1 || nper[w] > SURFDISP_NPER_MAX || pred_stride[k] < nper[w])) ok = false;
        }
    }
    if (ok && !pred[0] && !pred[2]) ok = false;
    if (ok && ellip && pred[4]) {                                           // chi [stacks][nper[0]] of the Rayleigh solve
        j.pred[4] = pred[4];
        j.pstride[4] = pred_stride[4];
        if (!pred[0] || pred_stride[4] < nper[0]) ok = false;
    }
    if (!ok) {
        set_err("%s: bad argument (1 <= nsteps <= depth <= 4, 1 <= Ptot <= 800, every given prediction array with 1 <= nper <= stride)", name);
        return SURFDISP_ERR_INVALID;
    }
    j.cols = cols;
    j.weights = weights;
    j.a = sd::McmcAcceptArgs{C, N, Ptot, nullptr, nullptr, obs, uncer, mask, obs_per_chain ? 1 : 0, p1, p0, chi0, row, row_stride,
                             seed, counter, first ? 1 : 0, chain0, depth, nsteps, step_stride};
    SD_HIP(sd::launch_mcmc_accept_joint(static_cast<hipStream_t>(stream), j, ellip));
    return SURFDISP_SUCCESS;
}

int surfdisp_mcmc_accept_joint_device(void *stream, int C, int N, const float *const pred[4], const long pred_stride[4],
                                      const int nper[2], const int *const status[2], int Ptot, const int *cols, const double *weights,
                                      const double *obs, const double *uncer, const unsigned char *mask, int obs_per_chain,
                                      const double *p1, double *p0, double *chi0, double *row, long row_stride,
                                      unsigned long long seed, unsigned long long counter, int first, long chain0)
{
    return mcmc_accept_joint("surfdisp_mcmc_accept_joint_device", false, stream, C, N, pred, pred_stride, nper, status, Ptot, cols, weights,
                             obs, uncer, mask, obs_per_chain, p1, p0, chi0, row, row_stride, 0, seed, counter, first, chain0, 1, 1);
}

int surfdisp_mcmc_accept_tree_joint_device(void *stream, int C, int N, int depth, int nsteps, const float *const pred[4],
                                           const long pred_stride[4], const int nper[2], const int *const status[2], int Ptot,
                                           const int *cols, const double *weights, const double *obs, const double *uncer,
                                           const unsigned char *mask, int obs_per_chain, const double *q, double *p0, double *chi0,
                                           double *row, long row_stride, long step_stride, unsigned long long seed,
                                           unsigned long long counter, long chain0)
{
    return mcmc_accept_joint("surfdisp_mcmc_accept_tree_joint_device", false, stream, C, N, pred, pred_stride, nper, status, Ptot, cols,
                             weights, obs, uncer, mask, obs_per_chain, q, p0, chi0, row, row_stride, step_stride, seed, counter, 0,
                             chain0, depth, nsteps);
}

// ... and with a fifth prediction array, the ellipticity of the Rayleigh solve (column sources 4: chi, 5: |chi|).
int surfdisp_mcmc_accept_joint5_device(void *stream, int C, int N, const float *const pred[5], const long pred_stride[5],
                                       const int nper[2], const int *const status[2], int Ptot, const int *cols, const double *weights,
                                       const double *obs, const double *uncer, const unsigned char *mask, int obs_per_chain,
                                       const double *p1, double *p0, double *chi0, double *row, long row_stride,
                                       unsigned long long seed, unsigned long long counter, int first, long chain0)
{
    return mcmc_accept_joint("surfdisp_mcmc_accept_joint5_device", true, stream, C, N, pred, pred_stride, nper, status, Ptot, cols, weights,
                             obs, uncer, mask, obs_per_chain, p1, p0, chi0, row, row_stride, 0, seed, counter, first, chain0, 1, 1);
}

int surfdisp_mcmc_accept_tree_joint5_device(void *stream, int C, int N, int depth, int nsteps, const float *const pred[5],
                                            const long pred_stride[5], const int nper[2], const int *const status[2], int Ptot,
                                            const int *cols, const double *weights, const double *obs, const double *uncer,
                                            const unsigned char *mask, int obs_per_chain, const double *q, double *p0, double *chi0,
                                            double *row, long row_stride, long step_stride, unsigned long long seed,
                                            unsigned long long counter, long chain0)
{
    return mcmc_accept_joint("surfdisp_mcmc_accept_tree_joint5_device", true, stream, C, N, pred, pred_stride, nper, status, Ptot, cols,
                             weights, obs, uncer, mask, obs_per_chain, q, p0, chi0, row, row_stride, step_stride, seed, counter, 0,
                             chain0, depth, nsteps);
}

// The arguments the two least-squares entries share (sections (6d), (6e)): checked and copied into `a`; `outputs`: the entry's
// required output pointers are all given.  false (and the error text set) for a bad argument.
static bool lsq_args(const char *name, sd::LsqArgs &a, int B, int Lmax, const int *nlay, const float *model,
                     const unsigned char *free_mask, int free_per_stack, int nfree_max,
                     const float *const part[15], const float *const pred[5], const long pred_stride[5], const int nper[2],
                     int N, const int *cols, const double *weights,
                     const double *obs, const double *uncer, const unsigned char *mask, int obs_per_stack,
                     const double *vp_slope, const double *rho_slope, int slope_per_stack,
                     double alpha, const double *Q, int q_per_stack, const double *lam, bool outputs)
{
    bool ok = B >= 1 && Lmax >= 1 && Lmax <= SURFDISP_NLAY_MAX && N >= 1 && N <= sd::SD_MCMC_JOINT_MAX_COLS &&
              nfree_max >= 1 && nfree_max <= sd::SD_LSQ_MAX_FREE && nfree_max <= Lmax &&
              model && part && pred && pred_stride && nper && cols && weights && obs && uncer && mask && lam && outputs &&
              alpha >= 0.0 && alpha <= 1.7976931348623157e308;
    for (int w = 0; ok && w < 2; ++w) {
        a.nper[w] = nper[w];
        if (!pred[2 * w] && pred[2 * w + 1]) ok = false;                  // a group array without the phase array of its solve
        for (int k = 2 * w; ok && k < 2 * w + 2; ++k) {
            a.pred[k] = pred[k];
            a.pstride[k] = pred_stride[k];
            if (pred[k] && (nper[w] < 1 || nper[w] > SURFDISP_NPER_MAX || pred_stride[k] < nper[w])) ok = false;
        }
    }
    if (ok && !pred[0] && !pred[2]) ok = false;
    if (ok && pred[4]) {                                                    // chi [B][nper[0]] of the Rayleigh solve
        a.pred[4] = pred[4];
        a.pstride[4] = pred_stride[4];
        if (!pred[0] || pred_stride[4] < nper[0]) ok = false;
    }
    for (int k = 0; ok && k < 5; ++k) {                                     // a source's partials need its predictions
        bool any = false;
        for (int q = 0; q < 3; ++q) { a.part[3 * k + q] = part[3 * k + q]; any = any || part[3 * k + q]; }
        if (any && !pred[k]) ok = false;
    }
    if (!ok) {
        set_err("%s: bad argument (B >= 1, 1 <= Lmax <= 200, 1 <= N <= 800, 1 <= nfree_max <= min(128, Lmax), alpha >= 0, "
                "required pointers, every given prediction array with 1 <= nper <= stride, partials only of sources with predictions)", name);
        return false;
    }
    a.B = B; a.Lmax = Lmax; a.N = N; a.nmax = nfree_max;
    a.nlay = nlay; a.model = model; a.free_mask = free_mask; a.free_per_stack = free_per_stack ? 1 : 0;
    a.cols = cols; a.weights = weights; a.obs = obs; a.uncer = uncer; a.mask = mask; a.obs_per_stack = obs_per_stack ? 1 : 0;
    a.vp_slope = vp_slope; a.rho_slope = rho_slope; a.slope_per_stack = slope_per_stack ? 1 : 0;
    a.alpha = alpha; a.Q = Q; a.q_per_stack = q_per_stack ? 1 : 0; a.lam = lam;
    return true;
}

// One damped least-squares step of the free layers' Vs of every stack (csrc/surfdisp_lsq.hip): the prediction arrays and the
// column table of the joint accept entries, plus the partial arrays of the kernel entries.
int surfdisp_lsq_step_device(void *stream, int B, int Lmax, const int *nlay, const float *model,
                             const unsigned char *free_mask, int free_per_stack, int nfree_max,
                             const float *const part[15], const float *const pred[5], const long pred_stride[5], const int nper[2],
                             int N, const int *cols, const double *weights,
                             const double *obs, const double *uncer, const unsigned char *mask, int obs_per_stack,
                             const double *vp_slope, const double *rho_slope, int slope_per_stack,
                             double alpha, const double *Q, int q_per_stack, const double *lam,
                             double *delta, double *stats, int *info)
{
    sd::LsqArgs a{};
    if (!lsq_args("surfdisp_lsq_step_device", a, B, Lmax, nlay, model, free_mask, free_per_stack, nfree_max, part, pred, pred_stride,
                  nper, N, cols, weights, obs, uncer, mask, obs_per_stack, vp_slope, rho_slope, slope_per_stack, alpha, Q, q_per_stack,
                  lam, delta && stats && info))
        return SURFDISP_ERR_INVALID;
    a.delta = delta; a.stats = stats; a.info = info;
    SD_HIP(sd::launch_lsq_step(static_cast<hipStream_t>(stream), a));
    return SURFDISP_SUCCESS;
}

// Posterior covariance and resolution of the same problem at the same point (section (6e)): the step's arguments up to lam.
int surfdisp_lsq_resolution_device(void *stream, int B, int Lmax, const int *nlay, const float *model,
                                   const unsigned char *free_mask, int free_per_stack, int nfree_max,
                                   const float *const part[15], const float *const pred[5], const long pred_stride[5], const int nper[2],
                                   int N, const int *cols, const double *weights,
                                   const double *obs, const double *uncer, const unsigned char *mask, int obs_per_stack,
                                   const double *vp_slope, const double *rho_slope, int slope_per_stack,
                                   double alpha, const double *Q, int q_per_stack, const double *lam,
                                   double *cov, double *res, double *sigma_post, double *sigma_data, double *rdiag,
                                   double *stats, int *info)
{
    sd::LsqArgs a{};
    if (!lsq_args("surfdisp_lsq_resolution_device", a, B, Lmax, nlay, model, free_mask, free_per_stack, nfree_max, part, pred,
                  pred_stride, nper, N, cols, weights, obs, uncer, mask, obs_per_stack, vp_slope, rho_slope, slope_per_stack, alpha, Q,
                  q_per_stack, lam, sigma_post && sigma_data && rdiag && stats && info))
        return SURFDISP_ERR_INVALID;
    a.cov = cov; a.res = res; a.sigma_post = sigma_post; a.sigma_data = sigma_data; a.rdiag = rdiag; a.stats = stats; a.info = info;
    SD_HIP(sd::launch_lsq_resolution(static_cast<hipStream_t>(stream), a));
    return SURFDISP_SUCCESS;
}

// The thickness-mode arguments of section (6h), checked and copied into `a` behind lsq_args; `outputs`: the mode outputs the
// entry requires with K > 0 are all given.
static bool lsq_mode_args(const char *name, sd::LsqArgs &a, int nfree_max, int K, const double *modes, int modes_per_stack,
                          const float *const part_h[5], const double *mode_scale, const double *mode_prior, const double *mode_y,
                          bool outputs)
{
    if (K < 0 || K > sd::SD_LSQ_MAX_MODES || nfree_max + K > sd::SD_LSQ_MAX_FREE + sd::SD_LSQ_MAX_MODES ||
        (K > 0 && !(modes && part_h && mode_scale && outputs))) {
        set_err("%s: bad thickness-mode argument (0 <= K <= 8, nfree_max + K <= 136, with K > 0: modes, part_h, mode_scale and "
                "the mode outputs)", name);
        return false;
    }
    a.K = K;
    if (K > 0) {
        a.modes = modes; a.modes_per_stack = modes_per_stack ? 1 : 0;
        for (int k = 0; k < 5; ++k) a.part_h[k] = part_h[k];
        a.mode_scale = mode_scale; a.mode_prior = mode_prior; a.mode_y = mode_y;
    }
    return true;
}

// The step with K thickness modes behind the Vs unknowns (section (6h)); K = 0 launches the kernel of (6d) itself.
int surfdisp_lsq_step_modes_device(void *stream, int B, int Lmax, const int *nlay, const float *model,
                                   const unsigned char *free_mask, int free_per_stack, int nfree_max,
                                   const float *const part[15], const float *const pred[5], const long pred_stride[5], const int nper[2],
                                   int N, const int *cols, const double *weights,
                                   const double *obs, const double *uncer, const unsigned char *mask, int obs_per_stack,
                                   const double *vp_slope, const double *rho_slope, int slope_per_stack,
                                   double alpha, const double *Q, int q_per_stack, const double *lam,
                                   int K, const double *modes, int modes_per_stack, const float *const part_h[5],
                                   const double *mode_scale, const double *mode_prior, const double *mode_y,
                                   double *delta, double *delta_y, double *stats, int *info)
{
    const char *name = "surfdisp_lsq_step_modes_device";
    sd::LsqArgs a{};
    if (!lsq_args(name, a, B, Lmax, nlay, model, free_mask, free_per_stack, nfree_max, part, pred, pred_stride, nper, N, cols, weights,
                  obs, uncer, mask, obs_per_stack, vp_slope, rho_slope, slope_per_stack, alpha, Q, q_per_stack, lam,
                  delta && stats && info) ||
        !lsq_mode_args(name, a, nfree_max, K, modes, modes_per_stack, part_h, mode_scale, mode_prior, mode_y, delta_y != nullptr))
        return SURFDISP_ERR_INVALID;
    a.delta = delta; a.delta_y = delta_y; a.stats = stats; a.info = info;
    SD_HIP(sd::launch_lsq_step(static_cast<hipStream_t>(stream), a));
    return SURFDISP_SUCCESS;
}

// ... and its covariance and resolution; K = 0 launches the kernel of (6e) itself.
int surfdisp_lsq_resolution_modes_device(void *stream, int B, int Lmax, const int *nlay, const float *model,
                                         const unsigned char *free_mask, int free_per_stack, int nfree_max,
                                         const float *const part[15], const float *const pred[5], const long pred_stride[5],
                                         const int nper[2], int N, const int *cols, const double *weights,
                                         const double *obs, const double *uncer, const unsigned char *mask, int obs_per_stack,
                                         const double *vp_slope, const double *rho_slope, int slope_per_stack,
                                         double alpha, const double *Q, int q_per_stack, const double *lam,
                                         int K, const double *modes, int modes_per_stack, const float *const part_h[5],
                                         const double *mode_scale, const double *mode_prior, const double *mode_y,
                                         double *cov, double *res, double *sigma_post, double *sigma_data, double *rdiag,
                                         double *sigma_post_y, double *sigma_data_y, double *rdiag_y, double *stats, int *info)
{
    const char *name = "surfdisp_lsq_resolution_modes_device";
    sd::LsqArgs a{};
    if (!lsq_args(name, a, B, Lmax, nlay, model, free_mask, free_per_stack, nfree_max, part, pred, pred_stride, nper, N, cols, weights,
                  obs, uncer, mask, obs_per_stack, vp_slope, rho_slope, slope_per_stack, alpha, Q, q_per_stack, lam,
                  sigma_post && sigma_data && rdiag && stats && info) ||
        !lsq_mode_args(name, a, nfree_max, K, modes, modes_per_stack, part_h, mode_scale, mode_prior, mode_y,
                       sigma_post_y && sigma_data_y && rdiag_y))
        return SURFDISP_ERR_INVALID;
    a.cov = cov; a.res = res; a.sigma_post = sigma_post; a.sigma_data = sigma_data; a.rdiag = rdiag;
    a.sigma_post_y = sigma_post_y; a.sigma_data_y = sigma_data_y; a.rdiag_y = rdiag_y; a.stats = stats; a.info = info;
    SD_HIP(sd::launch_lsq_resolution(static_cast<hipStream_t>(stream), a));
    return SURFDISP_SUCCESS;
}

// Jacobian of the params -> stack map for a static-structure model without a thermal layer (section (6i);
// csrc/surfdisp_lsq_params.hip): the leading Nu columns of params are the unknowns.
int surfdisp_params_jacobian_device(void *stream, int C, int N, int Nu, int L, const double *params,
                                    const int *idesc, const double *fdesc, double *layer, double *jac)
{
    if (C < 1 || N < 1 || Nu < 1 || Nu > N || Nu > sd::SD_PLSQ_MAX_UNKNOWNS || L < 2 || L > SURFDISP_NLAY_MAX ||
        !params || !idesc || !fdesc || !jac) {
        set_err("surfdisp_params_jacobian_device: bad argument (C >= 1, 1 <= Nu <= min(N, 64), 2 <= L <= 200, params, idesc, fdesc, jac)");
        return SURFDISP_ERR_INVALID;
    }
    sd::ParamsJacArgs a{C, N, Nu, L, params, idesc, fdesc, layer, jac};
    SD_HIP(sd::launch_params_jacobian(static_cast<hipStream_t>(stream), a));
    return SURFDISP_SUCCESS;
}

// One damped least-squares step of the model parameters of every stack (section (6i)): the row table of (6d), the thickness
// arrays of (6h), and jac of surfdisp_params_jacobian_device.
int surfdisp_lsq_step_params_device(void *stream, int B, int Lmax, const int *nlay, int Nu, const double *jac,
                                    const float *const part[15], const float *const part_h[5],
                                    const float *const pred[5], const long pred_stride[5], const int nper[2],
                                    int N, const int *cols, const double *weights,
                                    const double *obs, const double *uncer, const unsigned char *mask, int obs_per_stack,
                                    const unsigned char *free_mask, int free_per_stack,
                                    const double *scale, const double *prior_w, const double *prior_ref,
                                    const double *params, int Np, const double *lam,
                                    double *delta, double *stats, int *info, double *cov, double *sigma, double *logdet)
{
    sd::ParamLsqArgs a{};
    bool ok = B >= 1 && Lmax >= 1 && Lmax <= SURFDISP_NLAY_MAX && N >= 1 && N <= sd::SD_MCMC_JOINT_MAX_COLS &&
              Nu >= 1 && Nu <= sd::SD_PLSQ_MAX_UNKNOWNS && Np >= Nu && jac && part && part_h && pred && pred_stride && nper &&
              cols && weights && obs && uncer && mask && scale && params && lam && delta && stats && info && (!prior_w || prior_ref);
    for (int w = 0; ok && w < 2; ++w) {
        a.nper[w] = nper[w];
        if (!pred[2 * w] && pred[2 * w + 1]) ok = false;                  // a group array without the phase array of its solve
        for (int k = 2 * w; ok && k < 2 * w + 2; ++k) {
            a.pred[k] = pred[k];
            a.pstride[k] = pred_stride[k];
            if (pred[k] && (nper[w] < 1 || nper[w] > SURFDISP_NPER_MAX || pred_stride[k] < nper[w])) ok = false;
        }
    }
    if (ok && !pred[0] && !pred[2]) ok = false;
    if (ok && pred[4]) {                                                    // chi [B][nper[0]] of the Rayleigh solve
        a.pred[4] = pred[4];
        a.pstride[4] = pred_stride[4];
        if (!pred[0] || pred_stride[4] < nper[0]) ok = false;
    }
    for (int k = 0; ok && k < 5; ++k) {                                     // a source's partials need its predictions
        bool any = part_h[k] != nullptr;
        a.part_h[k] = part_h[k];
        for (int q = 0; q < 3; ++q) { a.part[3 * k + q] = part[3 * k + q]; any = any || part[3 * k + q]; }
        if (any && !pred[k]) ok = false;
    }
    if (!ok) {
        set_err("surfdisp_lsq_step_params_device: bad argument (B >= 1, 1 <= Lmax <= 200, 1 <= N <= 800, 1 <= Nu <= min(64, Np), "
                "required pointers - jac, part, part_h, scale, params among them -, prior_ref with prior_w, every given prediction array "
                "with 1 <= nper <= stride, partials only of sources with predictions)");
        return SURFDISP_ERR_INVALID;
    }
    a.B = B; a.Lmax = Lmax; a.N = N; a.Nu = Nu; a.Np = Np;
    a.nlay = nlay; a.jac = jac;
    a.cols = cols; a.weights = weights; a.obs = obs; a.uncer = uncer; a.mask = mask; a.obs_per_stack = obs_per_stack ? 1 : 0;
    a.free_mask = free_mask; a.free_per_stack = free_per_stack ? 1 : 0;
    a.scale = scale; a.prior_w = prior_w; a.prior_ref = prior_ref; a.params = params; a.lam = lam;
    a.delta = delta; a.stats = stats; a.info = info; a.cov = cov; a.sigma = sigma; a.logdet = logdet;
    SD_HIP(sd::launch_lsq_step_params(static_cast<hipStream_t>(stream), a));
    return SURFDISP_SUCCESS;
}

// Measurement variants that do NOT synchronise: the caller owns four events per call
// (surfdisp_events_create) which are recorded on the launch stream before prep, between the
// kernels and after finish; durations are read later with surfdisp_events_elapsed_ms, after the
// caller's own synchronisation.  This is what bench.py uses inside its timed region.
static int forward_with_events(void *stream, int B, int Lmax, const int *nlay,
                               const float *model, int P, const float *per, int kind,
                               float *c, float *u, float *ratio, int *status,
                               void *workspace, size_t workspace_bytes, void *const *events4)
{
    if (!events4) { set_err("events4 is NULL"); return SURFDISP_ERR_INVALID; }
    hipEvent_t ev[4];
    for (int i = 0; i < 4; ++i) ev[i] = static_cast<hipEvent_t>(events4[i]);
    ForwardOpts o;
    o.events = ev;
    o.ratio = ratio;
    return forward_device_impl(stream, B, Lmax, nlay, model, P, per, kind, c, u, status, workspace, workspace_bytes, o);
}

int surfdisp_forward_batch_device_events(void *stream, int B, int Lmax, const int *nlay,
                                         const float *model, int P, const float *per, int kind,
                                         float *c, float *u, int *status,
                                         void *workspace, size_t workspace_bytes, void *const *events4)
{
    return forward_with_events(stream, B, Lmax, nlay, model, P, per, kind, c, u, /* ratio */ nullptr, status, workspace, workspace_bytes, events4);
}

// ... of surfdisp_forward_batch_device2: the same events around the solve that also returns the ellipticity
int surfdisp_forward_batch_device2_events(void *stream, int B, int Lmax, const int *nlay,
                                          const float *model, int P, const float *per, int kind,
                                          float *c, float *u, float *ratio, int *status,
                                          void *workspace, size_t workspace_bytes, void *const *events4)
{
    return forward_with_events(stream, B, Lmax, nlay, model, P, per, kind, c, u, ratio, status, workspace, workspace_bytes, events4);
}

int surfdisp_events_create(int n, void **events)
{
    if (n < 0 || !events) { set_err("bad events array"); return SURFDISP_ERR_INVALID; }
    for (int i = 0; i < n; ++i) {
        hipEvent_t e;
        SD_HIP(hipEventCreate(&e));
        events[i] = e;
    }
    return SURFDISP_SUCCESS;
}

int surfdisp_events_destroy(int n, void **events)
{
    if (!events) return SURFDISP_ERR_INVALID;
    for (int i = 0; i < n; ++i) if (events[i]) (void)hipEventDestroy(static_cast<hipEvent_t>(events[i]));
    return SURFDISP_SUCCESS;
}

// make `stream` wait for `event` (recorded on another stream by surfdisp_forward_batch_device_events): lets a caller order
// the kernels of two solves on two streams, e.g. the Love root search behind the Rayleigh one while the Rayleigh
// group-velocity kernel fills the rest of the chip (forward.JointPlan)
int surfdisp_stream_wait_event(void *stream, void *event)
{
    if (!event) { set_err("NULL event"); return SURFDISP_ERR_INVALID; }
    SD_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(event), 0));
    return SURFDISP_SUCCESS;
}

int surfdisp_events_elapsed_ms(void *start, void *stop, float *ms)
{
    if (!start || !stop || !ms) { set_err("NULL event"); return SURFDISP_ERR_INVALID; }
    SD_HIP(hipEventElapsedTime(ms, static_cast<hipEvent_t>(start), static_cast<hipEvent_t>(stop)));
    return SURFDISP_SUCCESS;
}

// Measurement variant: same launches, bracketed by HIP events recorded ON THE LAUNCH STREAM;
// waits for completion and returns the three kernel durations in milliseconds
// (kernel_ms[0..2] = prep, phase, group).  Not capturable in a graph (it synchronises).
int surfdisp_forward_batch_device_timed(void *stream, int B, int Lmax, const int *nlay,
                                        const float *model, int P, const float *per, int kind,
                                        float *c, float *u, int *status,
                                        void *workspace, size_t workspace_bytes, float *kernel_ms)
{
    if (!kernel_ms) { set_err("kernel_ms is NULL"); return SURFDISP_ERR_INVALID; }
    hipEvent_t ev[4];
    for (int i = 0; i < 4; ++i) SD_HIP(hipEventCreate(&ev[i]));
    ForwardOpts o;
    o.events = ev;
    int rc = forward_device_impl(stream, B, Lmax, nlay, model, P, per, kind, c, u, status, workspace, workspace_bytes, o);
    if (rc == SURFDISP_SUCCESS) {
        hipError_t e = hipEventSynchronize(ev[3]);
        if (e != hipSuccess) { set_err("hipEventSynchronize failed: %s", hipGetErrorString(e)); rc = SURFDISP_ERR_HIP; }
        for (int i = 0; i < 3 && rc == SURFDISP_SUCCESS; ++i)
            if (hipEventElapsedTime(&kernel_ms[i], ev[i], ev[i + 1]) != hipSuccess) {
                set_err("hipEventElapsedTime failed"); rc = SURFDISP_ERR_HIP;
            }
    }
    for (int i = 0; i < 4; ++i) (void)hipEventDestroy(ev[i]);
    return rc;
}

// Small calls (the one-stack drop-in fast_surf_ above all) reuse a per-thread device arena and a pinned
// staging buffer: one host->device and one device->host copy per call instead of six, and no
// hipMalloc/hipFree.  Kept until the thread exits.
namespace {
constexpr size_t ARENA_MAX = (size_t)4 << 20;         // calls needing more go through hipMalloc
struct HostArena {
    int dev = -1;
    char *d = nullptr, *h = nullptr;
    size_t dcap = 0, hcap = 0;
    bool reserve(int device, size_t dbytes, size_t hbytes)
    {
        if (dev != device) { release(); dev = device; }
        if (dbytes > dcap) {
            if (d) (void)hipFree(d);
            d = nullptr; dcap = 0;
            if (hipMalloc(reinterpret_cast<void **>(&d), dbytes) != hipSuccess) return false;
            dcap = dbytes;
        }
        if (hbytes > hcap) {
            if (h) (void)hipHostFree(h);
            h = nullptr; hcap = 0;
            if (hipHostMalloc(reinterpret_cast<void **>(&h), hbytes, hipHostMallocDefault) != hipSuccess) return false;
            hcap = hbytes;
        }
        return true;
    }
    void release()
    {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        d = h = nullptr; dcap = hcap = 0;
    }
    // no destructor on purpose: at thread/process exit the HIP runtime may already be gone
};
thread_local HostArena g_arena;
}  // namespace

// Large host-buffer calls: a grow-only device buffer and three streams per calling thread (no hipMalloc / hipFree per
// call), the batch cut into chunks that take turns on the streams - chunk k+1's copy-in and chunk k-1's copy-out run
// beside chunk k's kernels, and consecutive chunks' kernels overlap as independent batches in flight do.  Measured
// (scripts/time_host_api.py, C call, host buffers in and out): 65 536 x L10 3.07 -> 2.26 ms (21 -> 29 M solves/s),
// 262 144 x L10 11.4 -> 7.7 ms (23 -> 34 M); slots 2 / 3 and chunks of 16 384 / 32 768 / 65 536 ten-layer stacks swept.
struct HostPipe {
    int dev = -1;
    char *d = nullptr;
    size_t cap = 0;
    hipStream_t s[3] = {nullptr, nullptr, nullptr};
    bool ensure(int device, size_t bytes)
    {
        if (dev != device) { release(); dev = device; }
        for (int i = 0; i < 3; ++i)
            if (!s[i] && hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking) != hipSuccess) return false;
        if (bytes > cap) {
            if (d) (void)hipFree(d);
            d = nullptr; cap = 0;
            if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) return false;
            cap = bytes;
        }
        return true;
    }
    void release()
    {
        if (d) (void)hipFree(d);
        for (int i = 0; i < 3; ++i) { if (s[i]) (void)hipStreamDestroy(s[i]); s[i] = nullptr; }
        d = nullptr; cap = 0;
    }
    // no destructor on purpose (see HostArena)
};
thread_local HostPipe g_pipe;
constexpr size_t PIPE_KEEP_MAX = (size_t)3 << 30;      // a larger buffer is given back after the call

// chunks of a large host-buffer call: about 327 680 layers' worth of stacks each (32 768 ten-layer stacks), at least two;
// stacks of more than 20 layers go through in one piece (16 384 x L64: 3.56 ms either way, 25 600 x L96: 8.65 against 9.35 ms)
static int host_chunks(int B, int Lmax)
{
    long bc = (long)knobs().host_chunk_layers / Lmax;
    if (bc < 16384) return 1;          // deep stacks: the copies are a tenth of the call and smaller launches cost more than they hide
    if (bc > 65536) bc = 65536;
    if (B < bc) return 1;
    const long n = (B + bc - 1) / bc;
    return (int)(n < 2 ? 2 : n);
}

static int forward_batch_pipelined(int device, int nch, int B, int Lmax, const int *nlay, const float *model,
                                   int P, const float *per, int kind, float *c, float *u, int *status)
{
    const int Bc = (int)((((long)B + nch - 1) / nch + 63) / 64 * 64);          // stacks per chunk (the last one may be shorter)
    const HostSlot h = host_slot(Bc, Lmax, P);
    const size_t slot = h.bytes;
    const int NS = knobs().host_slots >= 3 ? 3 : 2;
    if (!g_pipe.ensure(device, NS * slot)) { set_err("host-buffer pipeline: allocation failed"); return SURFDISP_ERR_HIP; }
    int ret = SURFDISP_SUCCESS;
    auto copy_out = [&](int k) -> bool {                   // chunk k's results to the caller's arrays (stream-ordered behind its kernels)
        char *d = g_pipe.d + (size_t)(k % NS) * slot;
        hipStream_t s = g_pipe.s[k % NS];
        const long b0 = (long)k * Bc;
        const size_t bc = (size_t)((B - b0) < Bc ? (B - b0) : Bc);
        return hipMemcpyAsync(c + b0 * P, d + h.o_c, bc * P * sizeof(float), hipMemcpyDeviceToHost, s) == hipSuccess &&
               (!u || hipMemcpyAsync(u + b0 * P, d + h.o_u, bc * P * sizeof(float), hipMemcpyDeviceToHost, s) == hipSuccess) &&
               (!status || hipMemcpyAsync(status + b0, d + h.o_st, bc * sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess);
    };
    int k = 0;
    for (; k < nch && ret == SURFDISP_SUCCESS; ++k) {
        char *d = g_pipe.d + (size_t)(k % NS) * slot;
        hipStream_t s = g_pipe.s[k % NS];
        const long b0 = (long)k * Bc;
        const int bc = (int)((B - b0) < Bc ? (B - b0) : Bc);
        if (bc <= 0) break;
        // the slot's previous chunk leaves first (a copy to pageable memory holds the calling thread until that chunk is
        // done - the other slot's chunk is computing meanwhile)
        if (k >= NS && !copy_out(k - NS)) { set_err("device->host copy failed"); ret = SURFDISP_ERR_HIP; break; }
        const bool ok = hipMemcpyAsync(d + h.o_model, model + (size_t)b0 * 5 * Lmax, (size_t)bc * 5 * Lmax * sizeof(float), hipMemcpyHostToDevice, s) == hipSuccess &&
                        (k >= NS || hipMemcpyAsync(d + h.o_per, per, h.np, hipMemcpyHostToDevice, s) == hipSuccess) &&
                        (!nlay || hipMemcpyAsync(d + h.o_nl, nlay + b0, (size_t)bc * sizeof(int), hipMemcpyHostToDevice, s) == hipSuccess);
        if (!ok) { set_err("host->device copy failed"); ret = SURFDISP_ERR_HIP; break; }
        ret = surfdisp_forward_batch_device(s, bc, Lmax, nlay ? h.at<int>(d, h.o_nl) : nullptr, h.at<float>(d, h.o_model), P,
                                            h.at<float>(d, h.o_per), kind | SURFDISP_PIPELINED, h.at<float>(d, h.o_c),
                                            u ? h.at<float>(d, h.o_u) : nullptr, h.at<int>(d, h.o_st), d + h.o_ws, h.ws);
    }
    if (ret == SURFDISP_SUCCESS) {
        for (int j = (k >= NS ? k - NS : 0); j < k; ++j)
            if (!copy_out(j)) { set_err("device->host copy failed"); ret = SURFDISP_ERR_HIP; break; }
    }
    for (int i = 0; i < NS; ++i) {
        hipError_t e = hipStreamSynchronize(g_pipe.s[i]);
        if (e != hipSuccess && ret == SURFDISP_SUCCESS) { set_err("kernel execution failed: %s", hipGetErrorString(e)); ret = SURFDISP_ERR_HIP; }
    }
    if (g_pipe.cap > PIPE_KEEP_MAX) g_pipe.release();
    return ret;
}

int surfdisp_forward_batch(int device, int B, int Lmax, const int *nlay, const float *model,
                           int P, const float *per, int kind,
                           float *c, float *u, int *status)
{
    int rc = check_args(B, Lmax, P, kind, model, per, c, u);
    if (rc) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        set_err("no HIP device: libsurfdisp_hip has no CPU fallback");
        return SURFDISP_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) { set_err("bad device ordinal"); return SURFDISP_ERR_INVALID; }
    // run on `device`, then hand the calling thread back the device it had selected
    struct DeviceScope {
        int prev = -1;
        ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
    } scope;
    if (hipGetDevice(&scope.prev) != hipSuccess) scope.prev = -1;
    if (scope.prev == device) scope.prev = -1;                 // nothing to restore
    else SD_HIP(hipSetDevice(device));
    const HostSlot hs = host_slot(B, Lmax, P);
    const bool small = hs.bytes <= ARENA_MAX;
    if (!small) {
        const int nch = knobs().host_pipeline ? host_chunks(B, Lmax) : 1;
        if (nch > 1) return forward_batch_pipelined(device, nch, B, Lmax, nlay, model, P, per, kind, c, u, status);
    }
    char *d = nullptr, *h = nullptr;
    hipStream_t s = nullptr;
    if (small) {
        if (!g_arena.reserve(device, hs.bytes, hs.o_ws)) { set_err("arena allocation failed"); return SURFDISP_ERR_HIP; }
        d = g_arena.d; h = g_arena.h;
    } else {
        if (!g_pipe.ensure(device, hs.bytes)) { set_err("host-buffer call: allocation failed"); return SURFDISP_ERR_HIP; }
        d = g_pipe.d; s = g_pipe.s[0];
    }
    int ret = SURFDISP_SUCCESS;
    do {
        bool ok;
        if (small) {
            memcpy(h + hs.o_model, model, hs.nm);
            memcpy(h + hs.o_per, per, hs.np);
            if (nlay) memcpy(h + hs.o_nl, nlay, hs.ni);
            ok = hipMemcpyAsync(d, h, hs.o_c, hipMemcpyHostToDevice, s) == hipSuccess;
        } else {
            ok = hipMemcpyAsync(d + hs.o_model, model, hs.nm, hipMemcpyHostToDevice, s) == hipSuccess &&
                 hipMemcpyAsync(d + hs.o_per, per, hs.np, hipMemcpyHostToDevice, s) == hipSuccess &&
                 (!nlay || hipMemcpyAsync(d + hs.o_nl, nlay, hs.ni, hipMemcpyHostToDevice, s) == hipSuccess);
        }
        if (!ok) { set_err("host->device copy failed"); ret = SURFDISP_ERR_HIP; break; }
        ret = surfdisp_forward_batch_device(s, B, Lmax, nlay ? hs.at<int>(d, hs.o_nl) : nullptr, hs.at<float>(d, hs.o_model), P,
                                            hs.at<float>(d, hs.o_per), kind, hs.at<float>(d, hs.o_c), hs.at<float>(d, hs.o_u),
                                            hs.at<int>(d, hs.o_st), d + hs.o_ws, hs.ws);
        if (ret) break;
        if (small) {
            ok = hipMemcpyAsync(h + hs.o_c, d + hs.o_c, hs.o_ws - hs.o_c, hipMemcpyDeviceToHost, s) == hipSuccess;
        } else {
            ok = hipMemcpyAsync(c, d + hs.o_c, hs.no, hipMemcpyDeviceToHost, s) == hipSuccess &&
                 (!u || hipMemcpyAsync(u, d + hs.o_u, hs.no, hipMemcpyDeviceToHost, s) == hipSuccess) &&
                 (!status || hipMemcpyAsync(status, d + hs.o_st, hs.ni, hipMemcpyDeviceToHost, s) == hipSuccess);
        }
        if (!ok) { set_err("device->host copy failed"); ret = SURFDISP_ERR_HIP; break; }
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) { set_err("kernel execution failed: %s", hipGetErrorString(e)); ret = SURFDISP_ERR_HIP; break; }
        if (small) {
            memcpy(c, h + hs.o_c, hs.no);
            if (u) memcpy(u, h + hs.o_u, hs.no);
            if (status) memcpy(status, h + hs.o_st, hs.ni);
        }
    } while (0);
    // an error exit may leave copies / kernels queued on the thread's cached stream that still write into the caller's pageable
    // arrays or into the buffer the next call reuses: drain it before returning (the result is the error already recorded)
    if (ret != SURFDISP_SUCCESS) (void)hipStreamSynchronize(s);
    if (!small && g_pipe.cap > PIPE_KEEP_MAX) g_pipe.release();
    return ret;
}

// frees what the host-buffer entries cached for the calling thread (device arena, pinned staging, pipeline buffer, streams)
void surfdisp_thread_release(void)
{
    g_arena.release();
    g_arena.dev = -1;
    g_pipe.release();
    g_pipe.dev = -1;
}

// Fortran-ABI drop-in for the reference object's symbol (fast_surf.f:2-5).
void fast_surf_(const int *n_layer, const int *kind,
                const float *vp, const float *vs, const float *rho,
                const float *h, const float *qsinv,
                const float *per, const int *nper,
                float *uR, float *uL, float *cR, float *cL)
{
    if (!n_layer || !kind || !nper || !vp || !vs || !rho || !h || !qsinv || !per) return;
    const int n = *n_layer, P = *nper > SURFDISP_NPER_MAX ? SURFDISP_NPER_MAX : *nper;  // init.f:63-66
    if (n < 2 || n > SURFDISP_NLAY_MAX || P < 1) { set_err("fast_surf_: bad n_layer/nper"); return; }
    float *model = static_cast<float *>(malloc((size_t)5 * n * sizeof(float)));
    float c[SURFDISP_NPER_MAX], u[SURFDISP_NPER_MAX];
    if (!model) return;
    memcpy(model + 0 * n, vp, n * sizeof(float));
    memcpy(model + 1 * n, vs, n * sizeof(float));
    memcpy(model + 2 * n, rho, n * sizeof(float));
    memcpy(model + 3 * n, h, n * sizeof(float));
    memcpy(model + 4 * n, qsinv, n * sizeof(float));
    const int dev = knobs().device;
    const int rc = surfdisp_forward_batch(dev, 1, n, nullptr, model, P, per, *kind, c, u, nullptr);
    free(model);
    if (rc != SURFDISP_SUCCESS) {
        // no silent fallback: report loudly and leave the outputs untouched (= all zeros = failure
        // in the reference's convention, models.py:29-33)
        fprintf(stderr, "surfdisp fast_surf_: %s\n", g_err);
        return;
    }
    for (int i = 0; i < P; ++i) {                       // fast_surf.f:197-208
        if (c[i] == 0.0f) break;
        if (*kind == SURFDISP_KIND_LOVE) { if (cL) cL[i] = c[i]; if (uL) uL[i] = u[i]; }
        else                             { if (cR) cR[i] = c[i]; if (uR) uR[i] = u[i]; }
    }
}

}  // extern "C"
