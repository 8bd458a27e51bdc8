// corrections.hip -- the derived coefficients of the Euler-pole correction (beat/models/corrections.py:90-140,
// heart.velocities_from_pole heart.py:4326-4392) and the coupling map built on them (ffi/fault.py:1436-1517).
//
// The pole term of a dataset is linear in three numbers per chain, coef = omega' p (ctx.hpp GeoCorrTerm, kind 1):
//     p      = ecef(pole_lat, pole_lon, 0) / r_earth        heart.py:4381-4383 (geodetic_to_ecef, the closed form)
//     omega' = omega * 1e-6 * (pi / 180) * r_earth          heart.py:4385
// k_pole_coef evaluates them for every (chain, pole term) in ONE order of operations, plain products and sums without
// contraction (tests/eulerpole_ref.py and models/corrections.py pole_coefficients restate it):
//     rlat = pole_lat * d2r ;  rlon = pole_lon * d2r ;  e2 = 2 f - f * f              d2r = pi / 180, f the oblateness
//     N    = a / sqrt(1 - e2 * (sin(rlat) * sin(rlat)))                               a the equatorial radius
//     px   = ((N * cos(rlat)) * cos(rlon)) / r ;  py = ((N * cos(rlat)) * sin(rlon)) / r
//     pz   = ((N * (1 - e2)) * sin(rlat)) / r                                         r the earth's radius
//     w    = ((omega * 1e-6) * d2r) * r ;  coef = (w * px, w * py, w * pz)
// The earth's three constants come with the term as data.  A lane per (chain, term): the work is a handful of
// transcendental calls per chain, one small launch in front of each kernel that subtracts corrections.
#include "kernels.hpp"

namespace beatamd {

__device__ __forceinline__ void pole_coef(double pole_lat, double pole_lon, double omega, double r, double a, double f,
                                          double *c0, double *c1, double *c2)
{
#pragma clang fp contract(off)
    const double d2r = 3.14159265358979323846 / 180.0;
    const double rlat = pole_lat * d2r, rlon = pole_lon * d2r;
    const double e2 = 2.0 * f - f * f;
    const double sl = sin(rlat), cl = cos(rlat), so = sin(rlon), co = cos(rlon);
    const double N = a / sqrt(1.0 - e2 * (sl * sl));
    const double px = ((N * cl) * co) / r, py = ((N * cl) * so) / r, pz = ((N * (1.0 - e2)) * sl) / r;
    const double w = ((omega * 1e-6) * d2r) * r;
    *c0 = w * px;
    *c1 = w * py;
    *c2 = w * pz;
}

__device__ __forceinline__ void pole_coef_of(const PoleTerm &t, const double *Qc, double *c0, double *c1, double *c2)
{
    const double lat = t.off[0] < 0 ? t.fix[0] : Qc[t.off[0]];
    const double lon = t.off[1] < 0 ? t.fix[1] : Qc[t.off[1]];
    const double om = t.off[2] < 0 ? t.fix[2] : Qc[t.off[2]];
    pole_coef(lat, lon, om, t.earth[0], t.earth[1], t.earth[2], c0, c1, c2);
}

// out [C, npole, 4]: record (c, j) = (coef0, coef1, coef2, 0)
__global__ void __launch_bounds__(256) k_pole_coef(const PoleTerm *terms, int npole, const double *Q, int64_t nparams, int64_t C,
                                                  double *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C * npole) return;
    const int64_t c = i / npole;
    const int j = (int)(i - c * npole);
    double c0, c1, c2;
    pole_coef_of(terms[j], Q + c * nparams, &c0, &c1, &c2);
    double *o = out + i * 4;
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = 0.0;
}

int launch_pole_coef(beatamd_ctx *ctx, const PoleTerm *terms, int npole, const double *Q, int64_t nparams, int64_t C, double *out)
{
    if (C == 0 || npole == 0) return BEATAMD_OK;
    const int64_t nb = (C * npole + 255) / 256;
    BA_CHECK(nb < (int64_t)0x7fffffff, BEATAMD_EINVAL, "pole_coef: batch too large");
    ScopedTimer tm(ctx, "pole_coef");
    hipLaunchKernelGGL(k_pole_coef, dim3((unsigned)nb), dim3(256), 0, ctx->stream, terms, npole, Q, nparams, C, out);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// fault.py:1497 euler_slips = |sum_k Bp[i,k] coef_k| (the sum in the order of geo_corr_subtract), :1514-1517
// coupling = 100 * clip(uparr / euler_slips, 0, 1) with numpy's semantics: a NaN ratio stays NaN, x / 0 -> inf -> 100.
// Lane <-> (draw, patch); every lane derives its draw's coefficients itself (no second buffer, no order between calls)
__global__ void __launch_bounds__(256) k_pole_coupling(PoleTerm term, const double *Q, int64_t nparams, int64_t C, int64_t P,
                                                      const double *Bp, int64_t uparr_off, double *euler_slips, double *coupling)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C * P) return;
    const int64_t c = i / P, p = i - c * P;
    const double *Qc = Q + c * nparams;
    double c0, c1, c2;
    pole_coef_of(term, Qc, &c0, &c1, &c2);
    const double *B = Bp + p * 3;
    const double es = fabs((B[0] * c0 + B[1] * c1) + B[2] * c2);
    double r = Qc[uparr_off + p] / es;
    r = r < 0.0 ? 0.0 : r;
    r = r > 1.0 ? 1.0 : r;
    euler_slips[i] = es;
    coupling[i] = r * 100.0;
}

int launch_pole_coupling(beatamd_ctx *ctx, const PoleTerm &term, const double *Q, int64_t nparams, int64_t C, int64_t P,
                         const double *Bp, int64_t uparr_off, double *euler_slips, double *coupling)
{
    if (C * P == 0) return BEATAMD_OK;
    const int64_t nb = (C * P + 255) / 256;
    BA_CHECK(nb < (int64_t)0x7fffffff, BEATAMD_EINVAL, "pole_coupling: batch too large");
    ScopedTimer tm(ctx, "pole_coupling");
    hipLaunchKernelGGL(k_pole_coupling, dim3((unsigned)nb), dim3(256), 0, ctx->stream, term, Q, nparams, C, P, Bp, uparr_off,
                       euler_slips, coupling);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
