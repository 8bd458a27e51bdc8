// philox.hpp -- the random draws of the sampler kernels (smc.hip, hyper.hip) as device functions: the counter-based
// generator and, per stream, the one function that turns its blocks into a draw.  Every kernel that draws calls
// these -- the step-by-step kernels (k_philox_normal, k_philox_chain, k_philox_univariate) and the fused ones
// (k_draw_propose, k_hyper_chain) alike -- so the same counters give the same bits on every path.  What a step does
// with a draw (propose, box test, accept, tune) is metropolis.hpp.
#pragma once
#include <cstdint>

#include "ctx.hpp"

#ifdef __HIPCC__
namespace beatamd {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
// SC'11) -- counter-based, so a draw is a pure function of (seed, step, chain, element): the
// proposal rows of a chain do not depend on how chains are sharded over GPUs.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 53-bit uniform in (0, 1): ((hi >> 5) * 2^26 + (lo >> 6) + 0.5) * 2^-53
__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo)
{
    return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6) + 0.5) * (1.0 / 9007199254740992.0);
}

// a pair of standard normals from one block: (cos, sin) of the same radius and angle
__device__ __forceinline__ void box_muller(const uint32_t (&r)[4], double &a, double &b)
{
    const double u1 = u53(r[0], r[1]), u2 = u53(r[2], r[3]);
    const double rad = sqrt(-2.0 * log(u1));
    const double th = 6.283185307179586476925286766559 * u2;
    a = rad * cos(th);
    b = rad * sin(th);
}

// counter layout: (pair index inside the row, global chain id, step, stream); key = seed
//   stream 0: proposal normals z[c, 2j], z[c, 2j+1] from pair j of chain c (box_muller; the callers draw the block)
//   stream 1: the row scale 1 / sqrt(chi2(df) / df) of a multivariate-t proposal with df degrees of freedom
//             (base.py:35-71): chi2 as the sum of df squared normals, two per block
__device__ __forceinline__ double philox_t_row_scale(uint32_t gc, uint32_t step, int df, uint32_t k0, uint32_t k1)
{
    double x = 0.0;
    for (int m = 0; m < df; m += 2) {
        uint32_t r[4];
        philox4x32_10((uint32_t)(m / 2), gc, step, 1u, k0, k1, r);
        double g0, g1;
        box_muller(r, g0, g1);
        x += g0 * g0;
        if (m + 1 < df) x += g1 * g1;
    }
    return 1.0 / sqrt(x / (double)df);
}

//   stream 2: Metropolis uniforms -- log u of chain gc at `step`
__device__ __forceinline__ double philox_log_u(uint32_t gc, uint32_t step, uint32_t k0, uint32_t k1)
{
    uint32_t r[4];
    philox4x32_10(0u, gc, step, 2u, k0, k1, r);
    return log(u53(r[0], r[1]));
}

// streams 3 / 4: the unit draws (2j, 2j + 1) of a row of a per-parameter proposal family (reference
// beat/sampler/base.py:129-147), before the parameter's scale
//   kind 0  NormalProposal   Box-Muller pair
//   kind 1  CauchyProposal   standard_cauchy() = tan(pi (u - 1/2))
//   kind 2  LaplaceProposal  standard_exponential() - standard_exponential(), E = -log u
__device__ __forceinline__ void philox_univariate_pair(int kind, uint32_t j, uint32_t gc, uint32_t step, uint32_t k0,
                                                       uint32_t k1, double &a, double &b)
{
    uint32_t r[4];
    philox4x32_10(j, gc, step, 3u, k0, k1, r);
    if (kind == 0) {
        box_muller(r, a, b);
    } else if (kind == 1) {
        const double u1 = u53(r[0], r[1]), u2 = u53(r[2], r[3]);
        a = tan(3.14159265358979323846 * (u1 - 0.5));
        b = tan(3.14159265358979323846 * (u2 - 0.5));
    } else {
        const double u1 = u53(r[0], r[1]), u2 = u53(r[2], r[3]);
        uint32_t q[4];
        philox4x32_10(j, gc, step, 4u, k0, k1, q);
        a = log(u53(q[0], q[1])) - log(u1);     // E1 - E2 with E = -log u
        b = log(u53(q[2], q[3])) - log(u2);
    }
}

// Poisson variate from ONE uniform by inversion (sequential search from k = 0, pmf recurrence p_k = p_{k-1} lam / k).
// Exact in law while exp(-lam) is a normal double; step widths lam <= 500 only: a wider one (or NaN) raises
// ST_BAD_SCALE -> BEATAMD_EINVAL at the next synchronisation (the host side refuses it beforehand,
// beat_amd/sampler/metropolis.py) and the draw is NaN.  The search stops where the cumulative sum stops growing (a
// uniform above the rounded sum, ~1e-13 of the draws at lam near 500, lands on that far-tail k instead of the search cap).
__device__ __forceinline__ double poisson_from_uniform(double u, double lam, int *status)
{
    if (lam == 0.0) return 0.0;
    if (!(lam > 0.0 && lam <= 500.0)) {
        atomicOr(status, ST_BAD_SCALE);
        return __builtin_nan("");
    }
    double p = exp(-lam), F = p;
    int k = 0;
    while (u > F && k < 4096) {
        k++;
        p *= lam / (double)k;
        const double Fn = F + p;
        if (Fn == F && (double)k > lam) break;
        F = Fn;
    }
    return (double)k;
}

// the scaled steps (2j, 2j + 1) of a row of any per-parameter family (base.py:129-160: every component is an
// independent draw times the parameter's scale):
//   kind 0..2  philox_univariate_pair times the scales sa, sb
//   kind 3     PoissonProposal  poisson(lam = scale) - scale, both uniforms from the stream-3 block (base.py:150-155;
//              integer steps around zero mean)
// A row of odd length has no component 2j + 1 in its last pair: the caller passes sb = 0.0 there and drops b.
__device__ __forceinline__ void philox_scaled_pair(int kind, uint32_t j, uint32_t gc, uint32_t step, uint32_t k0,
                                                   uint32_t k1, double sa, double sb, int *status, double &a, double &b)
{
    if (kind == 3) {
        uint32_t r[4];
        philox4x32_10(j, gc, step, 3u, k0, k1, r);
        const double u1 = u53(r[0], r[1]), u2 = u53(r[2], r[3]);
        a = poisson_from_uniform(u1, sa, status) - sa;
        b = poisson_from_uniform(u2, sb, status) - sb;
        return;
    }
    philox_univariate_pair(kind, j, gc, step, k0, k1, a, b);
    a = a * sa;
    b = b * sb;
}

}  // namespace beatamd
#endif
