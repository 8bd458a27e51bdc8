// mechanisms.hip -- the arrays behind the mechanism-ensemble figures of a moment-tensor run: `beat plot fuzzy_beachball`,
// `fuzzy_mt_decomp` and `hudson` (beat/plotting/seismic.py:1334-1425 lower_focalsphere_angles / mts2amps, :1664-1850
// fuzzy_mt_decomposition, :2183-2310 draw_hudson).  The per-draw arithmetic is mechanism.hpp's.
//
// What the kernels promise:
//   k_mt_check      the smallest row index of X with a non-finite entry or (m6 input) all six entries zero
//   k_mt_decompose  one lane per draw, registers only; a draw's numbers depend on its own row alone, so how a population is
//                   cut into calls changes no bit
//   k_fuzzy_accum   MASK: count [P, npix] += #{draws of the chunk with a > 0} by one integer atomic per pixel and chunk:
//                   exact, whatever the order.  !MASK: sum [P, npix] = the amplitudes of ALL draws added in ascending
//                   index order into one accumulator per pixel (no split over draws): independent of the tiling.
//                   a = ((((r0 u0 + r1 u1) + r2 u2) + r3 u3) + r4 u4) + r5 u5, plain products and sums in this order;
//                   an amplitude of exactly 0, below 0 or NaN counts nothing (seismic.py:1419-1421).
//   k_fuzzy_finish  amps [P, ny nx] = NaN everywhere, then count / n (sum / n) at pixel_index
#include <hip/hip_runtime.h>

#include "ctx.hpp"
#include "devmath.hpp"
#include "kernels.hpp"
#include "mechanism.hpp"

namespace beatamd {

namespace {

constexpr int MC_TB = 256;

// *bad = min(*bad, first bad row) (set to 0xffffffff by the caller)
__global__ void __launch_bounds__(MC_TB) k_mt_check(const double *X, int64_t n, int w, int zero_is_bad, uint32_t *bad)
{
    const int64_t i = (int64_t)blockIdx.x * MC_TB + threadIdx.x;
    if (i >= n) return;
    bool fin = true, zero = true;
    for (int k = 0; k < w; k++) {
        const double x = X[i * w + k];
        fin = fin && is_finite(x);
        zero = zero && x == 0.0;
    }
    if (!fin || (zero && zero_is_bad)) atomicMin(bad, (uint32_t)i);
}

// X [n, 6] tensors (kind 0) or [n, 3] strike, dip, rake in degrees (kind 1); every output is nullable
__global__ void __launch_bounds__(MC_TB) k_mt_decompose(int64_t n, int kind, const double *X, double *evals, double *evecs,
                                                       double *moments, double *ratios, double *parts, double *unit,
                                                       double *uv)
{
    const int64_t i = (int64_t)blockIdx.x * MC_TB + threadIdx.x;
    if (i >= n) return;
    double m[6];
    if (kind == 1) {
        mech_dc_m6(X[3 * i], X[3 * i + 1], X[3 * i + 2], m);
    } else {
#pragma unroll
        for (int k = 0; k < 6; k++) m[k] = X[6 * i + k];
    }
    MechDraw r;
    mech_draw(m, r);
    if (evals) {
#pragma unroll
        for (int k = 0; k < 3; k++) evals[3 * i + k] = r.evals[k];
    }
    if (evecs) {
#pragma unroll
        for (int k = 0; k < 9; k++) evecs[9 * i + k] = r.evecs[k / 3][k % 3];
    }
    if (moments) {
#pragma unroll
        for (int k = 0; k < MECH_NPART; k++) moments[MECH_NPART * i + k] = r.moments[k];
    }
    if (ratios) {
#pragma unroll
        for (int k = 0; k < MECH_NPART; k++) ratios[MECH_NPART * i + k] = r.ratios[k];
    }
    if (parts) {
#pragma unroll
        for (int k = 0; k < MECH_NPART * 6; k++) parts[MECH_NPART * 6 * i + k] = r.parts[k / 6][k % 6];
    }
    if (unit) {
#pragma unroll
        for (int k = 0; k < MECH_NPART * 6; k++) unit[MECH_NPART * 6 * i + k] = r.unit[k / 6][k % 6];
    }
    if (uv) {
        uv[2 * i] = r.uv[0];
        uv[2 * i + 1] = r.uv[1];
    }
}

// Tile blockIdx.x (G TB consecutive pixels, lane-major: pixel = tile base + g TB + thread), draws [blockIdx.y chunk,
// + chunk) and part blockIdx.z of unit [n, P, 6].  A lane keeps the six weights of each of its G pixels in registers; the
// tensor of a draw sits at a wavefront-uniform address (kernel arguments, block indices and the loop counter only), so it
// comes through the scalar data cache and costs the vector pipe nothing.  Two shapes: wide (G = 4, TB = 256) where the
// tiles fill the device, narrow (G = 1, TB = 64) where they would not; the same bits in both.
template <int G, int TB, bool MASK>
__global__ void __launch_bounds__(TB) k_fuzzy_accum(int64_t n, int P, const double *__restrict__ unit, int64_t npix,
                                                      const double *__restrict__ rw, int64_t chunk, uint32_t *count,
                                                      double *sum)
{
#pragma clang fp contract(off)
    const int part = blockIdx.z;
    const int64_t base = (int64_t)blockIdx.x * (G * TB);
    const int64_t i0 = (int64_t)blockIdx.y * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
    double r[G][6], acc[G];
    uint32_t cnt[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        int64_t px = base + (int64_t)g * TB + threadIdx.x;
        if (px >= npix) px = npix - 1;   // a spare lane repeats the last pixel and stores nothing
#pragma unroll
        for (int k = 0; k < 6; k++) r[g][k] = rw[k * npix + px];
        acc[g] = 0.0;
        cnt[g] = 0u;
    }
    const double *u = unit + ((int64_t)i0 * P + part) * 6;
    const int64_t stride = (int64_t)P * 6;
#pragma unroll 4
    for (int64_t i = i0; i < i1; i++, u += stride) {
        const double u0 = u[0], u1 = u[1], u2 = u[2], u3 = u[3], u4 = u[4], u5 = u[5];
#pragma unroll
        for (int g = 0; g < G; g++) {
            const double a = ((((r[g][0] * u0 + r[g][1] * u1) + r[g][2] * u2) + r[g][3] * u3) + r[g][4] * u4) + r[g][5] * u5;
            if (MASK) cnt[g] += a > 0.0 ? 1u : 0u;
            else acc[g] += a;
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
        const int64_t px = base + (int64_t)g * TB + threadIdx.x;
        if (px < npix) {
            if (MASK) {
                if (cnt[g]) atomicAdd(&count[(int64_t)part * npix + px], cnt[g]);
            } else {
                sum[(int64_t)part * npix + px] = acc[g];
            }
        }
    }
}

__global__ void __launch_bounds__(MC_TB) k_fuzzy_fill(double *amps, int64_t total)
{
    const int64_t e = (int64_t)blockIdx.x * MC_TB + threadIdx.x;
    if (e < total) amps[e] = __builtin_nan("");
}

// amps [P, cells]: pixel j of part blockIdx.y -> cell pixel_index[j] (checked by the caller to lie in [0, cells))
__global__ void __launch_bounds__(MC_TB) k_fuzzy_finish(int64_t n, int64_t npix, const int64_t *pixel_index, int64_t cells,
                                                       const uint32_t *count, const double *sum, double *amps)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * MC_TB + threadIdx.x, p = blockIdx.y;
    if (j >= npix) return;
    const double v = count ? (double)count[p * npix + j] : sum[p * npix + j];
    amps[p * cells + pixel_index[j]] = v / (double)n;
}

}  // namespace

// ================================================================================================ launchers
int launch_mt_check(beatamd_ctx *ctx, const double *X, int64_t n, int kind, uint32_t *bad)
{
    BA_HIP(hipMemsetAsync(bad, 0xff, sizeof(uint32_t), ctx->stream));
    if (n == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_mt_check, dim3((unsigned)((n + MC_TB - 1) / MC_TB)), dim3(MC_TB), 0, ctx->stream, X, n,
                       kind == 1 ? 3 : 6, kind == 0, bad);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_mt_decompose(beatamd_ctx *ctx, int64_t n, int kind, const double *X, double *evals, double *evecs, double *moments,
                        double *ratios, double *parts, double *unit, double *uv)
{
    if (n == 0) return BEATAMD_OK;
    ScopedTimer tm(ctx, "mt_decompose");
    hipLaunchKernelGGL(k_mt_decompose, dim3((unsigned)((n + MC_TB - 1) / MC_TB)), dim3(MC_TB), 0, ctx->stream, n, kind, X, evals,
                       evecs, moments, ratios, parts, unit, uv);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_fuzzy_amps(beatamd_ctx *ctx, int64_t n, int P, const double *unit, int64_t npix, const double *rw,
                      const int64_t *pixel_index, int64_t cells, int mask, int shape, uint32_t *count, double *sum, double *amps)
{
    if (P == 0 || cells == 0) return BEATAMD_OK;
    const int64_t total = (int64_t)P * cells;
    BA_CHECK((total + MC_TB - 1) / MC_TB < (int64_t)0x7fffffff && P <= 65535, BEATAMD_EINVAL, "fuzzy_amps: grid too large");
    hipLaunchKernelGGL(k_fuzzy_fill, dim3((unsigned)((total + MC_TB - 1) / MC_TB)), dim3(MC_TB), 0, ctx->stream, amps, total);
    if (npix > 0) {
        const int64_t chunk = mask ? MC_CHUNK : n, nchunk = (n + chunk - 1) / chunk;
        const int64_t wide_tiles = (npix + MC_TILE - 1) / MC_TILE;
        // wide where its workgroups give every compute unit two, narrow below; shape 1 / 2 force wide / narrow
        const bool wide = shape == 1 || (shape != 2 && wide_tiles * nchunk * P >= 512);
        const int64_t ntile = wide ? wide_tiles : (npix + 63) / 64;
        BA_CHECK(ntile < (int64_t)0x7fffffff && nchunk <= 65535, BEATAMD_EINVAL, "fuzzy_amps: batch too large");
        ScopedTimer tm(ctx, mask ? "fuzzy_count" : "fuzzy_sum");
        const dim3 grid((unsigned)ntile, (unsigned)nchunk, (unsigned)P);
        if (mask) {
            BA_HIP(hipMemsetAsync(count, 0, (size_t)P * npix * sizeof(uint32_t), ctx->stream));
            if (wide)
                hipLaunchKernelGGL((k_fuzzy_accum<MC_G, MC_TB, true>), grid, dim3(MC_TB), 0, ctx->stream, n, P, unit, npix, rw,
                                   chunk, count, sum);
            else
                hipLaunchKernelGGL((k_fuzzy_accum<1, 64, true>), grid, dim3(64), 0, ctx->stream, n, P, unit, npix, rw, chunk,
                                   count, sum);
        } else {
            if (wide)
                hipLaunchKernelGGL((k_fuzzy_accum<MC_G, MC_TB, false>), grid, dim3(MC_TB), 0, ctx->stream, n, P, unit, npix, rw,
                                   chunk, count, sum);
            else
                hipLaunchKernelGGL((k_fuzzy_accum<1, 64, false>), grid, dim3(64), 0, ctx->stream, n, P, unit, npix, rw, chunk,
                                   count, sum);
        }
        hipLaunchKernelGGL(k_fuzzy_finish, dim3((unsigned)((npix + MC_TB - 1) / MC_TB), (unsigned)P), dim3(MC_TB), 0, ctx->stream,
                           n, npix, pixel_index, cells, mask ? count : nullptr, sum, amps);
    }
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
