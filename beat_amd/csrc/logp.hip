// logp.hip -- the small kernels around the two heavy ones: likelihood epilogues (`like` of a row and
// LOG_2PI: metropolis.hpp), the geodetic static stacking, noise covariance estimation.  All O(C * small).
#include "kernels.hpp"
#include "metropolis.hpp"

namespace beatamd {

__device__ __forceinline__ double hp_value(const HpSrc &h, int64_t c, int64_t d)
{
    return h.base[c * h.stride + (h.offs ? h.offs[d] : d)];
}

// distributions.py:119-138:
//   -0.5 * (slog_pdet + M*(2*hp + log_2pi) + (1/exp(hp*2)) * dot(tmp,tmp)),  M cast to int16
__global__ void __launch_bounds__(256) k_mvn_finish(int64_t C, int64_t nd, int64_t M,
                                                   const double *quad, const double *slog,
                                                   HpSrc hp, double *logpts, int64_t ld)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C * nd) return;
    const int64_t c = i / nd, d = i - c * nd;
    const double h = hp_value(hp, c, d);
    const double norm = (double)(int16_t)M * (2 * h + LOG_2PI);
    logpts[c * ld + d] = (-0.5) * (slog[d] + norm + (1 / exp(h * 2)) * quad[i]);
}

int launch_mvn_finish(beatamd_ctx *ctx, int64_t C, int64_t nd, int64_t M, const double *quad,
                      const double *slog, HpSrc hp, double *logpts, int64_t ld)
{
    const int64_t n = C * nd;
    if (n == 0) return BEATAMD_OK;
    ScopedTimer tm(ctx, "finish");
    hipLaunchKernelGGL(k_mvn_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       C, nd, M, quad, slog, hp, logpts, ld);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// one wavefront per (c,d): quad = sum_k (w_d x_k)^2
__global__ void __launch_bounds__(256) k_scalar_quad(int64_t C, int64_t nd, int64_t M,
                                                    const double *X, int64_t xs_c, int64_t xs_d,
                                                    const double *w, double *quad)
{
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= C * nd) return;
    const int64_t c = i / nd, d = i - c * nd;
    const double *x = X + c * xs_c + d * xs_d;
    const double wd = w[d];
    double q = 0.0;
    for (int64_t k = lane; k < M; k += 64) {
        const double t = wd * x[k];
        q = fma(t, t, q);
    }
    for (int off = 32; off > 0; off >>= 1) q += __shfl_down(q, off, 64);   // wave_tree<OpAdd> (wave.hpp); the call changes the code
    if (lane == 0) quad[i] = q;
}

int launch_scalar_quad(beatamd_ctx *ctx, int64_t C, int64_t nd, int64_t M, const double *X,
                       int64_t xs_c, int64_t xs_d, const double *w, double *quad)
{
    const int64_t n = C * nd;
    if (n == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_scalar_quad, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, C,
                       nd, M, X, xs_c, xs_d, w, quad);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ffi/base.py:292-305  mu = G.T.dot(slips), summed over the slip variables (geodetic.py:1065-1070): block (CH chains,
// 128 observation points), the chains' slips in LDS as [variable][p][CH]; an element of G is read once per CH chains and
// sixteen loads are in flight per lane (round 6: one chain per block read the 1.4 MB of G 512 times per call, one launch
// per slip variable with mu through memory in between: 2 x 58 us at 512 chains x 428 points x 400 patches).  Per (chain,
// point) the same fma sequence -- variables ascending, patches ascending -- as the one-chain kernel: bitwise equal.
struct GeoStackArgs {
    const double *G[4];
    ChainVec slips[4];
    int nvar, accumulate;
    int64_t P, Nobs, C;
    double *mu;
};

template <int CH>
__global__ void __launch_bounds__(256) k_geo_stack(GeoStackArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_slip[];
    const int64_t c0 = (int64_t)blockIdx.y * CH;
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t P = a.P, Nobs = a.Nobs;
    for (int v = 0; v < a.nvar; v++)
        for (int64_t i = threadIdx.x; i < P * CH; i += blockDim.x) {
            const int64_t p = i / CH, j = i % CH;
            s_slip[v * P * CH + i] = c0 + j < a.C ? a.slips[v].base[(c0 + j) * a.slips[v].stride + a.slips[v].off + p] : 0.0;
        }
    __syncthreads();
    if (k >= Nobs) return;
    double acc[CH];
#pragma unroll
    for (int j = 0; j < CH; j++) acc[j] = (a.accumulate && c0 + j < a.C) ? a.mu[(c0 + j) * Nobs + k] : 0.0;
    for (int v = 0; v < a.nvar; v++) {
        const double *G = a.G[v] + k;
        const double *sl = s_slip + v * P * CH;
        // two groups of sixteen loads of G in flight per lane: the next group is requested before the group in hand is
        // used (a block is two wavefronts; the loop is a row of round trips to L2, nothing else covers them)
        int64_t p = 0;
        double ga[16], gb[16];
        const int64_t nfull = P / 16;
        if (nfull > 0) {
#pragma unroll
            for (int u = 0; u < 16; u++) ga[u] = G[u * Nobs];
        }
        for (int64_t ch = 0; ch < nfull; ch += 2) {
            if (ch + 1 < nfull) {
#pragma unroll
                for (int u = 0; u < 16; u++) gb[u] = G[(p + 16 + u) * Nobs];
            }
#pragma unroll
            for (int u = 0; u < 16; u++)
#pragma unroll
                for (int j = 0; j < CH; j++) acc[j] = fma(ga[u], sl[(p + u) * CH + j], acc[j]);
            p += 16;
            if (ch + 1 < nfull) {
                if (ch + 2 < nfull) {
#pragma unroll
                    for (int u = 0; u < 16; u++) ga[u] = G[(p + 16 + u) * Nobs];
                }
#pragma unroll
                for (int u = 0; u < 16; u++)
#pragma unroll
                    for (int j = 0; j < CH; j++) acc[j] = fma(gb[u], sl[(p + u) * CH + j], acc[j]);
                p += 16;
            }
        }
        for (; p < P; p++) {
            const double g = G[p * Nobs];
#pragma unroll
            for (int j = 0; j < CH; j++) acc[j] = fma(g, sl[p * CH + j], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < CH; j++)
        if (c0 + j < a.C) a.mu[(c0 + j) * Nobs + k] = acc[j];
}

int launch_geo_stack(beatamd_ctx *ctx, const GeoLib *const *libs, int nvar, int64_t C, const ChainVec *slips, int accumulate,
                     double *mu)
{
    if (C == 0 || nvar == 0) return BEATAMD_OK;
    BA_CHECK(nvar >= 1 && nvar <= 4, BEATAMD_EINVAL, "geo_stack: 1..4 slip variables");
    const GeoLib &lib = *libs[0];
    if (nvar > 1 && (size_t)lib.P * nvar * sizeof(double) > 64 * 1024) {
        // (faults of more than 8192 / nvar patches: the variables' slips do not fit the block's LDS together -- one launch per
        // variable, mu through memory; the same fma sequence)
        for (int v = 0; v < nvar; v++) BA_TRY(launch_geo_stack(ctx, libs + v, 1, C, slips + v, (v > 0 || accumulate) ? 1 : 0, mu));
        return BEATAMD_OK;
    }
    GeoStackArgs a;
    for (int v = 0; v < nvar; v++) {
        BA_CHECK(libs[v]->P == lib.P && libs[v]->Nobs == lib.Nobs, BEATAMD_EINVAL, "geo_stack: the libraries of the slip variables differ in shape");
        a.G[v] = libs[v]->g.get();
        a.slips[v] = slips[v];
    }
    a.nvar = nvar; a.accumulate = accumulate;
    a.P = lib.P; a.Nobs = lib.Nobs; a.C = C;
    a.mu = mu;
    ScopedTimer tm(ctx, "geostack");
    const int CH = (C >= 64 && (size_t)lib.P * nvar * 4 * sizeof(double) <= 64 * 1024) ? 4 : 1;
    const size_t lds = (size_t)lib.P * nvar * CH * sizeof(double);
    BA_CHECK(lds <= 64 * 1024, BEATAMD_EINVAL, "geo_stack: more than 8192 patch slips per chain");
    BA_CHECK((C + CH - 1) / CH <= 65535, BEATAMD_EINVAL, "geo_stack: at most %d chains per call", 65535 * CH);
    const dim3 grid((unsigned)((lib.Nobs + 127) / 128), (unsigned)((C + CH - 1) / CH));
    if (CH == 4) hipLaunchKernelGGL(k_geo_stack<4>, grid, dim3(128), lds, ctx->stream, a);
    else hipLaunchKernelGGL(k_geo_stack<1>, grid, dim3(128), lds, ctx->stream, a);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// geodetic.py:1072-1074: (sdata - mu) * sodws ; :1076-1077 apply_corrections where the composite has terms (the
// branch on gc.nterm is the same for every thread of the launch)
__global__ void __launch_bounds__(256) k_geo_residual(int64_t C, int64_t Nobs, const double *data,
                                                     const double *odw, const double *mu,
                                                     double *res, const double *Q, int64_t nparams, GeoCorr gc)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C * Nobs) return;
    const int64_t k = i % Nobs;
    if (gc.nterm > 0)
        res[i] = geo_corrected_residual(gc, Q, nparams, i / Nobs, k, data[k], mu[i], odw[k]);
    else
        res[i] = (data[k] - mu[i]) * odw[k];
}

int launch_geo_residual(beatamd_ctx *ctx, int64_t C, int64_t Nobs, const double *data,
                        const double *odw, const double *mu, double *res, const double *Q,
                        int64_t nparams, GeoCorr gc)
{
    const int64_t n = C * Nobs;
    if (n == 0) return BEATAMD_OK;
    BA_CHECK(gc.nterm == 0 || (Q && C <= 2147483647), BEATAMD_EINVAL, "geo_residual: corrections need q and fewer than 2^31 chains");
    hipLaunchKernelGGL(k_geo_residual, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       ctx->stream, C, Nobs, data, odw, mu, res, Q, nparams, gc);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// laplacian.py:88-96 _eval_prior summed over slip variables (:126-139)
__global__ void __launch_bounds__(256) k_laplacian_finish(int64_t C, int64_t nvar, int64_t P,
                                                         double logdet, const double *quad,
                                                         HpSrc hp, double *out, int64_t ld)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double h = hp_value(hp, c, 0);
    double s = 0.0;
    for (int64_t v = 0; v < nvar; v++)
        s += (-0.5) * (-logdet + ((double)P * (LOG_2PI + 2 * h)) +
                       (1.0 / exp(h * 2) * quad[c * nvar + v]));
    out[c * ld] = s;
}

int launch_laplacian_finish(beatamd_ctx *ctx, int64_t C, int64_t nvar, int64_t P, double logdet,
                            const double *quad, HpSrc hp, double *out, int64_t ld)
{
    if (C == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_laplacian_finish, dim3((unsigned)((C + 255) / 256)), dim3(256), 0,
                       ctx->stream, C, nvar, P, logdet, quad, hp, out, ld);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// update_llks (seismic.py:510-525, geodetic.py:429-444, laplacian.py:141-154) for a batch: the quadratic forms the
// likelihood kernels left in `quad` go into their columns of llks [C, nterm] as they are
__global__ void __launch_bounds__(256) k_store_misfits(int64_t C, int64_t n, const double *src, double *dst, int64_t ld)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C * n) return;
    const int64_t c = i / n, k = i - c * n;
    dst[c * ld + k] = src[i];
}

int launch_store_misfits(beatamd_ctx *ctx, int64_t C, int64_t n, const double *src, double *dst, int64_t ld)
{
    if (C * n == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_store_misfits, dim3((unsigned)((C * n + 255) / 256)), dim3(256), 0, ctx->stream, C, n, src, dst, ld);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// a chain whose times left the library grid: NaN in all its columns (as its `like` in k_like_sum)
__global__ void __launch_bounds__(256) k_misfits_mark_bad(int64_t C, int64_t n, double *llks, const int32_t *chain_bad)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C * n) return;
    if (chain_bad[i / n]) llks[i] = __builtin_nan("");
}

int launch_misfits_mark_bad(beatamd_ctx *ctx, int64_t C, int64_t n, double *llks, const int32_t *chain_bad)
{
    if (C * n == 0 || !chain_bad) return BEATAMD_OK;
    hipLaunchKernelGGL(k_misfits_mark_bad, dim3((unsigned)((C * n + 255) / 256)), dim3(256), 0, ctx->stream, C, n, llks, chain_bad);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// problems.py:227-247: like = sum over composites of (composite llk vector).sum()  (like_serial, metropolis.hpp)
__global__ void __launch_bounds__(256) k_like_sum(int64_t C, int64_t nllk, LikeGroups grp,
                                                 double *LL, const int32_t *chain_bad)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double *l = LL + c * nllk;
    l[nllk - 1] = like_serial(l, grp, chain_bad && chain_bad[c]);
}

int launch_like_sum(beatamd_ctx *ctx, int64_t C, int64_t nllk, const LikeGroups &grp, double *LL,
                    const int32_t *chain_bad)
{
    if (C == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_like_sum, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, ctx->stream, C,
                       nllk, grp, LL, chain_bad);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// Likelihood vectors of a model whose seismic targets are SHARDED over ranks (beat_amd/models/sharded.py; SURVEY 8(e):
// "each GPU owns T/R targets for all chains ... one small collective"): the all-gathered block `src` [nsrc, C] holds,
// rank by rank, the rows a rank contributes -- the logpts of its datasets (dst_col[r] = their column in the full vector)
// and one flag row per rank (dst_col[r] = -1: NaN marks a chain whose times left the library grid on one of THAT rank's
// targets).  Thread <-> chain: scatter the rows into LL [C, nllk], copy the replicated columns (geodetic, Laplacian) from
// this rank's local vector, then `like` as k_like_sum takes it (like_serial) -- from the same gathered bits on every rank.
__global__ void __launch_bounds__(256) k_like_assemble(int64_t C, int64_t nllk, int64_t nsrc, const double *src,
                                                      const int32_t *dst_col, const double *rest, int64_t rest_ld,
                                                      int64_t rest_col0, int64_t n_rest, int64_t rest_dst0, LikeGroups grp,
                                                      double *LL, int32_t *chain_bad)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double *l = LL + c * nllk;
    bool bad = false;
    for (int64_t r = 0; r < nsrc; r++) {
        const double v = src[r * C + c];
        const int32_t d = dst_col[r];
        if (d >= 0) l[d] = v;
        else bad = bad || (v != v);
    }
    for (int64_t k = 0; k < n_rest; k++) l[rest_dst0 + k] = rest[c * rest_ld + rest_col0 + k];
    l[nllk - 1] = like_serial(l, grp, bad);
    if (chain_bad) chain_bad[c] = bad ? 1 : 0;
}

int launch_like_assemble(beatamd_ctx *ctx, int64_t C, int64_t nllk, int64_t nsrc, const double *src, const int32_t *dst_col,
                         const double *rest, int64_t rest_ld, int64_t rest_col0, int64_t n_rest, int64_t rest_dst0,
                         const LikeGroups &grp, double *LL, int32_t *chain_bad)
{
    if (C == 0) return BEATAMD_OK;
    ScopedTimer tm(ctx, "finish");
    hipLaunchKernelGGL(k_like_assemble, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, ctx->stream, C, nllk, nsrc, src,
                       dst_col, rest, rest_ld, rest_col0, n_rest, rest_dst0, grp, LL, chain_bad);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

struct GatherArgs {
    ChainVec slips[4];
};
__global__ void __launch_bounds__(256) k_gather_slips(int64_t C, int nvar, int64_t P, GatherArgs g,
                                                     double *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C * nvar * P) return;
    const int64_t p = i % P;
    const int64_t cv = i / P;
    const int v = (int)(cv % nvar);
    const int64_t c = cv / nvar;
    out[i] = g.slips[v].base[c * g.slips[v].stride + g.slips[v].off + p];
}

int launch_gather_slips(beatamd_ctx *ctx, int64_t C, int nvar, int64_t P, const ChainVec *slips,
                        double *out)
{
    GatherArgs g;
    for (int v = 0; v < nvar; v++) g.slips[v] = slips[v];
    const int64_t n = C * nvar * P;
    if (n == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_gather_slips, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       C, nvar, P, g, out);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ---------------------------------------------------------------- noise covariance estimation
// numpy's float64 sum of a contiguous row, so that sum / n is numpy.mean(row) to the bit (the reference's
// data.mean(), covariance.py:730): numpy's pairwise_sum applied to pieces of at most 8192 elements (the
// reduction's buffer size), the pieces added in order to 0.0.  pairwise_sum: below 8 elements a plain loop from
// 0.0; up to 128 eight strided accumulators, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail; above
// that the two halves split at n/2 rounded down to a multiple of 8.
__device__ double np_block_sum(const double *a, int64_t n)
{
    double res = 0.0;
    if (n < 8) {
        for (int64_t i = 0; i < n; i++) res += a[i];
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; j++) r[j] = a[j];
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; j++) r[j] += a[i + j];
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += a[i];
    return res;
}

// the recursion unrolled by depth: a half is at most n/2 + 8 long, so a piece of 8192 reaches blocks of <= 128
// after 7 halvings (D = 8 leaves one to spare; pairwise_sum<0> is never reached with more than 128)
template <int D> __device__ __attribute__((noinline)) double np_pairwise_sum(const double *a, int64_t n)
{
    if (n <= 128) return np_block_sum(a, n);
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum<D - 1>(a, n2) + np_pairwise_sum<D - 1>(a + n2, n - n2);
}
template <> __device__ double np_pairwise_sum<0>(const double *a, int64_t n) { return np_block_sum(a, n); }

// covariance.py:716-736 autocovariance: autocov[j] = (1/n) sum_k (d[j+k]-m)(d[k]-m).  One thread
// per lag walks k in the reference's order with separate multiply and add (no contraction), so the
// result is bitwise the reference's O(n^2) Python loop; the trace sits in LDS.  mean == nullptr (device
// traces): thread 0 takes the row's mean from LDS in numpy's order first.
__global__ void __launch_bounds__(256) k_autocovariance(const double *data, int64_t n,
                                                       const double *mean, double *out)
{
    extern __shared__ __attribute__((aligned(16))) double s_d[];
    __shared__ double s_mean;
    const int64_t d = blockIdx.y;
    const double *x = data + d * n;
    if (mean) {
        if (threadIdx.x == 0) s_mean = mean[d];
    } else {
        for (int64_t k = threadIdx.x; k < n; k += 256) s_d[k] = x[k];
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int64_t c = 0; c < n; c += 8192) s += np_pairwise_sum<8>(s_d + c, n - c < 8192 ? n - c : 8192);
            s_mean = s / (double)n;
        }
    }
    __syncthreads();
    const double m = s_mean;
    for (int64_t k = threadIdx.x; k < n; k += 256) s_d[k] = x[k] - m;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double a = 0.0;
    for (int64_t k = 0; k < n - j; k++) a += s_d[j + k] * s_d[k];
    out[d * n + j] = a / (double)n;
}

int launch_autocovariance(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *data,
                          const double *mean, double *out)
{
    if (nd == 0 || n == 0) return BEATAMD_OK;
    BA_CHECK(n * 8 <= 150 * 1024, BEATAMD_EINVAL, "autocovariance: trace longer than 19200 samples");
    BA_CHECK(nd <= 65535, BEATAMD_EINVAL, "autocovariance: too many datasets");
    const size_t lds = (size_t)n * sizeof(double);
    if (lds > 64 * 1024)
        BA_HIP(hipFuncSetAttribute((const void *)k_autocovariance,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_autocovariance, dim3((unsigned)((n + 255) / 256), (unsigned)nd), dim3(256),
                       lds, ctx->stream, data, n, mean, out);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// covariance.py:739-771: C[i,j] = coeffs[|i-j|] * stds[i] * stds[j]
__global__ void __launch_bounds__(256) k_scaled_toeplitz(int64_t nd, int64_t n, const double *coeffs,
                                                        const double *stds, double *out)
{
    const int64_t total = nd * n * n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t c = i % n, r = (i / n) % n, d = i / (n * n);
        const int64_t l = r > c ? r - c : c - r;
        out[i] = coeffs[d * n + l] * stds[d * n + r] * stds[d * n + c];
    }
}

int launch_scaled_toeplitz(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *coeffs,
                           const double *stds, double *out)
{
    const int64_t total = nd * n * n;
    if (total == 0) return BEATAMD_OK;
    const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(k_scaled_toeplitz, dim3(grid), dim3(256), 0, ctx->stream, nd, n, coeffs, stds,
                       out);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
