// surfdisp_mcmc_rng.h -- the random streams of the Metropolis kernels: Philox4x32-10, the 53-bit uniform and the bounded Gaussian
// step, shared by surfdisp_mcmc.hip (propose, tree, masked redraw, accept) and surfdisp_mcmc_prior.hip (the redraw loop of a
// sampler with a prior).  The functions stand here as they stood in surfdisp_mcmc.hip; tests/mcmc_replay.py restates them on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sd {

struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(U4 ctr, uint32_t k0, uint32_t k1)
{
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, ctr.x), lo0 = M0 * ctr.x;
        const uint32_t hi1 = __umulhi(M1, ctr.z), lo1 = M1 * ctr.z;
        ctr = U4{hi1 ^ ctr.y ^ k0, lo1, hi0 ^ ctr.w ^ k1, lo0};
        k0 += W0; k1 += W1;
    }
    return ctr;
}
// uniform in (0, 1) from 53 random bits (never 0 nor 1)
__device__ __forceinline__ double u53(uint32_t a, uint32_t b)
{
    const uint64_t v = (((uint64_t)a << 32) | b) >> 11;
    return ((double)v + 0.5) * (1.0 / 9007199254740992.0);
}

// Bounded Gaussian step around x (brownian.py:20-27 BrownianVar.move): redrawn while it falls outside (lo, hi), at most 1000
// tries (two normals per Philox call), then a uniform draw ("No valid perturb, uniform reset instead!"); reset: the uniform
// branch at once (MCinv.reset).  node: position in the speculative tree (0 for the plain lock step).
__device__ __forceinline__ double draw_bounded(double x, double lo, double hi, double s, uint32_t k0, uint32_t k1,
                                               unsigned long long counter, uint32_t node, long gidx, bool reset)
{
    const uint32_t chi32 = (uint32_t)(counter >> 32) ^ (node << 20);
    double nv = 0.0;
    bool ok = false;
    for (uint32_t t = 0; t < 500 && !ok && !reset; ++t) {
        const U4 r = philox4x32_10(U4{(uint32_t)counter, chi32 ^ (t << 8), (uint32_t)gidx, (uint32_t)(gidx >> 32)}, k0, k1);
        const double u1 = u53(r.x, r.y), u2 = u53(r.z, r.w);
        const double rad = sqrt(-2.0 * log(u1));
        double sn, cs;
        sincospi(2.0 * u2, &sn, &cs);
        nv = x + s * rad * cs;
        ok = (nv < hi) && (nv > lo);
        if (!ok) { nv = x + s * rad * sn; ok = (nv < hi) && (nv > lo); }
    }
    if (!ok) {
        const U4 r = philox4x32_10(U4{(uint32_t)counter, chi32 ^ 0x00ffff00u, (uint32_t)gidx, (uint32_t)(gidx >> 32)}, k0, k1);
        nv = lo + (hi - lo) * u53(r.x, r.y);
    }
    return nv;
}

}  // namespace sd
