// philox.hpp -- device functions shared by the sampler kernels (smc.hip, hyper.hip): the counter-based generator,
// the transforms of the per-parameter proposal families and the step-size table.  One definition each, so that a
// kernel that fuses a whole chain draws and tunes bit for bit what the step-by-step kernels do.
#pragma once
#include <cstdint>

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

__device__ __forceinline__ void box_muller(const uint32_t (&r)[4], double &a, double &b)
{
    const double u1 = u53(r[0], r[1]), u2 = u53(r[2], r[3]);
    const double rad = sqrt(-2.0 * log(u1));
    const double th = 6.283185307179586476925286766559 * u2;
    a = rad * cos(th);
    b = rad * sin(th);
}

// counter layout: (pair index inside the row, global chain id, step, stream); key = seed
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

// metropolis.py:294-306 with pymc's tune table (restated from its documentation):
//   acc < 0.001 x0.1 | < 0.05 x0.5 | < 0.2 x0.9 | > 0.95 x10 | > 0.75 x2 | > 0.5 x1.1
__device__ __forceinline__ double tune_factor(double acc)
{
    double f = 1.0;
    if (acc < 0.001) f = 0.1;
    else if (acc < 0.05) f = 0.5;
    else if (acc < 0.2) f = 0.9;
    else if (acc > 0.95) f = 10.0;
    else if (acc > 0.75) f = 2.0;
    else if (acc > 0.5) f = 1.1;
    return f;
}

}  // namespace beatamd
#endif
