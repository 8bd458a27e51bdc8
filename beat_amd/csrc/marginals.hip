// marginals.hip -- the arrays behind the marginal-posterior plots of a population or trace X [n, V] (row-major):
// sorted columns, percentiles and histogram counts (plotting/common.py:248-397, marginals.py:131-507), pairwise 2-d
// counts (common.py:400-415) and pairwise gaussian kernel density estimates on a grid (common.py:445-461).
//
// What the kernels promise:
//   k_col_sort_*       values only, ascending; -0.0 and 0.0 compare equal and keep no order among themselves
//   k_col_percentiles  numpy.percentile's "linear" method, operation for operation (no contraction)
//   k_col_hist         integer counts from positions in the sorted column: exact, no atomics
//   k_pair_hist2d      integer atomics only: exact, whatever the order
//   k_pair_moments     sums in one fixed order (thread t adds samples t, t + TB, ... ascending, then block_sum_ldstree)
//   k_pair_kde2d       ONE accumulator per grid point, samples added in ascending index order: Z[p, a, b] does not depend
//                      on the tiling, on the pairs of the call or on the launch.  A skipped sample block holds exact zeros.
#include <hip/hip_runtime.h>

#include "ctx.hpp"
#include "devmath.hpp"
#include "kernels.hpp"
#include "wave.hpp"

namespace beatamd {

namespace {

constexpr int MG_SORT_TB = 1024;   // threads of a sorting workgroup
constexpr int MG_TB = 256;         // threads of every other workgroup here
constexpr double MG_INF = __builtin_huge_val();

// ---------------------------------------------------------------------------------------------- finite check
// flags[k] = 1 where column cols[k] of X holds a non-finite sample (flags zeroed by the caller; every writer stores 1)
__global__ void __launch_bounds__(MG_TB) k_col_check(const double *X, int64_t n, int64_t V, const int64_t *cols, int32_t *flags)
{
    const int64_t k = blockIdx.y;
    const double *x = X + cols[k];
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * MG_TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * MG_TB)
        bad = bad || !is_finite(x[i * V]);
    if (bad) flags[k] = 1;
}

// ---------------------------------------------------------------------------------------------- column sort
// The bitonic network in its one-direction form: a merge of blocks of size k starts with the flip (i against i ^ (k - 1))
// and goes on with the strides k/4, ..., 1 (i against i ^ s); every comparator puts the smaller value at the lower index.
// Positions >= n count as +inf: no comparator ever moves them, so they are never stored.
__device__ __forceinline__ void mg_cmpx(double &a, double &b)
{
    if (b < a) {
        const double t = a;
        a = b;
        b = t;
    }
}

// the strides s = s0, s0/2, ..., 1 of a merge inside the tile sh [L] (L a power of two, all threads of the workgroup)
__device__ __forceinline__ void mg_tile_strides(double *sh, int L, int s0)
{
    for (int s = s0; s > 0; s >>= 1) {
        for (int t = threadIdx.x; t < L / 2; t += MG_SORT_TB) {
            const int i = ((t & ~(s - 1)) << 1) | (t & (s - 1));
            mg_cmpx(sh[i], sh[i | s]);
        }
        __syncthreads();
    }
}

// mode 0: gather tile blockIdx.x of column cols[k] of X, sort it, write it to out [K, n];
// mode 1: the strides L/2 .. 1 of a merge on tile blockIdx.x of out
__global__ void __launch_bounds__(MG_SORT_TB) k_col_sort_tile(const double *X, int64_t n, int64_t V, const int64_t *cols,
                                                            double *out, int L, int mode)
{
    extern __shared__ __attribute__((aligned(16))) double mg_sh[];
    const int64_t k = blockIdx.y, base = (int64_t)blockIdx.x * L;
    double *o = out + k * n;
    if (mode == 0) {
        const double *x = X + cols[k];
        for (int t = threadIdx.x; t < L; t += MG_SORT_TB) mg_sh[t] = base + t < n ? x[(base + t) * V] : MG_INF;
    } else {
        for (int t = threadIdx.x; t < L; t += MG_SORT_TB) mg_sh[t] = base + t < n ? o[base + t] : MG_INF;
    }
    __syncthreads();
    if (mode == 0) {
        for (int kk = 2; kk <= L; kk <<= 1) {
            for (int t = threadIdx.x; t < L / 2; t += MG_SORT_TB) {
                const int h = kk >> 1;
                const int i = ((t & ~(h - 1)) << 1) | (t & (h - 1));
                mg_cmpx(mg_sh[i], mg_sh[i ^ (kk - 1)]);
            }
            __syncthreads();
            mg_tile_strides(mg_sh, L, kk >> 2);
        }
    } else {
        mg_tile_strides(mg_sh, L, L >> 1);
    }
    for (int t = threadIdx.x; t < L; t += MG_SORT_TB)
        if (base + t < n) o[base + t] = mg_sh[t];
}

// one comparator per thread on out [K, n] across tiles: flip != 0: i against i ^ (kk - 1) (h = kk / 2), else i against i ^ h
__global__ void __launch_bounds__(MG_TB) k_col_sort_global(double *out, int64_t n, int64_t npad, int64_t h, int flip)
{
    const int64_t t = (int64_t)blockIdx.x * MG_TB + threadIdx.x;
    if (t >= npad / 2) return;
    const int64_t i = ((t & ~(h - 1)) << 1) | (t & (h - 1));
    const int64_t j = flip ? (i ^ (2 * h - 1)) : (i | h);
    if (j >= n) return;   // +inf stays where it is
    double *o = out + (int64_t)blockIdx.y * n;
    double a = o[i], b = o[j];
    if (b < a) {
        o[i] = b;
        o[j] = a;
    }
}

// ---------------------------------------------------------------------------------------------- percentiles
// numpy's _quantile with method "linear" and its _lerp (numpy/lib/_function_base_impl.py)
__global__ void __launch_bounds__(MG_TB) k_col_percentiles(const double *S, int64_t K, int64_t n, const double *q, int64_t Q,
                                                          double *out)
{
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * MG_TB + threadIdx.x;
    if (e >= K * Q) return;
    const int64_t k = e / Q;
    const double *s = S + k * n;
    const double vi = (double)(n - 1) * (q[e - k * Q] / 100.0);
    int64_t lo = (int64_t)floor(vi), hi;
    const double t = vi - (double)lo;
    if (vi >= (double)(n - 1)) lo = hi = n - 1;
    else if (vi < 0.0) lo = hi = 0;
    else hi = lo + 1;
    const double a = s[lo], b = s[hi], d = b - a;
    out[e] = t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

// ---------------------------------------------------------------------------------------------- histograms
// counts[k, i] = #{edges[k, i] <= x < edges[k, i + 1]}, the last bin closed on the right (numpy.histogram)
__global__ void __launch_bounds__(MG_TB) k_col_hist(const double *S, int64_t n, const double *edges, int64_t nb, int64_t *counts)
{
    const int64_t i = (int64_t)blockIdx.x * MG_TB + threadIdx.x, k = blockIdx.y;
    if (i >= nb) return;
    const double *s = S + k * n, *e = edges + k * (nb + 1);
    const int64_t a = sorted_bound(s, n, e[i], false);
    const int64_t b = sorted_bound(s, n, e[i + 1], i + 1 == nb);
    counts[k * nb + i] = b - a;
}

// searchsorted(e, x, 'right') - 1 on the edges e [m + 1] in LDS, a value on the last edge in the last bin; -1: outside
__device__ __forceinline__ int mg_bin(const double *e, int m, double x)
{
    if (!(x >= e[0]) || !(x <= e[m])) return -1;
    int lo = 0, hi = m + 1;   // first index with e[i] > x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1 >= m ? m - 1 : lo - 1;
}

// counts [P, bx, by] += the samples blockIdx.y, blockIdx.y + gridDim.y, ... (in blocks of MG_TB) of pair blockIdx.x
__global__ void __launch_bounds__(MG_TB) k_pair_hist2d(const double *X, int64_t n, int64_t V, const int64_t *pairs, int bx, int by,
                                                      const double *xedges, const double *yedges, unsigned long long *counts)
{
    extern __shared__ __attribute__((aligned(16))) double mg_sh[];
    const int64_t p = blockIdx.x;
    double *ex = mg_sh, *ey = mg_sh + (bx + 1);
    uint32_t *g = reinterpret_cast<uint32_t *>(mg_sh + (bx + 1) + (by + 1));
    for (int t = threadIdx.x; t <= bx; t += MG_TB) ex[t] = xedges[p * (bx + 1) + t];
    for (int t = threadIdx.x; t <= by; t += MG_TB) ey[t] = yedges[p * (by + 1) + t];
    for (int t = threadIdx.x; t < bx * by; t += MG_TB) g[t] = 0u;
    __syncthreads();
    const double *x = X + pairs[2 * p], *y = X + pairs[2 * p + 1];
    for (int64_t i = (int64_t)blockIdx.y * MG_TB + threadIdx.x; i < n; i += (int64_t)gridDim.y * MG_TB) {
        const int a = mg_bin(ex, bx, x[i * V]), b = mg_bin(ey, by, y[i * V]);
        if (a >= 0 && b >= 0) atomicAdd(&g[a * by + b], 1u);
    }
    __syncthreads();
    unsigned long long *c = counts + p * (int64_t)bx * by;
    for (int t = threadIdx.x; t < bx * by; t += MG_TB)
        if (g[t]) atomicAdd(&c[t], (unsigned long long)g[t]);
}

// ---------------------------------------------------------------------------------------------- pair moments
// mom [P, MG_NMOM]: mean x, mean y, sum (x - mx)^2, sum (x - mx)(y - my), sum (y - my)^2, min x, max x, min y, max y
__global__ void __launch_bounds__(MG_TB) k_pair_moments(const double *X, int64_t n, int64_t V, const int64_t *pairs, double *mom)
{
#pragma clang fp contract(off)
    __shared__ double red[MG_TB];
    const int64_t p = blockIdx.x;
    const double *x = X + pairs[2 * p], *y = X + pairs[2 * p + 1];
    double sx = 0.0, sy = 0.0, xl = MG_INF, xh = -MG_INF, yl = MG_INF, yh = -MG_INF;
    for (int64_t i = threadIdx.x; i < n; i += MG_TB) {
        const double a = x[i * V], b = y[i * V];
        sx += a;
        sy += b;
        xl = fmin(xl, a); xh = fmax(xh, a);
        yl = fmin(yl, b); yh = fmax(yh, b);
    }
    const double mx = block_sum_ldstree<MG_TB>(sx, red) / (double)n;
    const double my = block_sum_ldstree<MG_TB>(sy, red) / (double)n;
    double sxx = 0.0, sxy = 0.0, syy = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += MG_TB) {
        const double a = x[i * V] - mx, b = y[i * V] - my;
        sxx += a * a;
        sxy += a * b;
        syy += b * b;
    }
    sxx = block_sum_ldstree<MG_TB>(sxx, red);
    sxy = block_sum_ldstree<MG_TB>(sxy, red);
    syy = block_sum_ldstree<MG_TB>(syy, red);
    xl = block_max_waveorder(-xl, red);   // min = -max(-x): exact
    xh = block_max_waveorder(xh, red);
    yl = block_max_waveorder(-yl, red);
    yh = block_max_waveorder(yh, red);
    if (threadIdx.x == 0) {
        double *m = mom + p * MG_NMOM;
        m[0] = mx; m[1] = my; m[2] = sxx; m[3] = sxy; m[4] = syy;
        m[5] = -xl; m[6] = xh; m[7] = -yl; m[8] = yh;
    }
}

// ---------------------------------------------------------------------------------------------- pair KDE
// W [P, n] = the samples of a pair centred, then whitened by the lower Cholesky factor L of its scaled covariance:
// u = (x - mx) / l11, v = ((y - my) - l21 u) / l22.  box [P, nblk, 4] = (min u, max u, min v, max v) of every block of
// MG_KDE_SB samples.  One workgroup per (sample block, pair); pairs with par.ok == 0 are left alone.
__global__ void __launch_bounds__(MG_TB) k_pair_whiten(const double *X, int64_t n, int64_t V, const int64_t *pairs,
                                                      const KdePair *par, double2 *W, double *box)
{
#pragma clang fp contract(off)
    __shared__ double red[MG_TB / 64];
    const int64_t p = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;
    const KdePair q = par[p];
    if (!q.ok) return;
    const double *x = X + pairs[2 * p], *y = X + pairs[2 * p + 1];
    double ul = MG_INF, uh = -MG_INF, vl = MG_INF, vh = -MG_INF;
    for (int e = threadIdx.x; e < MG_KDE_SB; e += MG_TB) {
        const int64_t i = blk * MG_KDE_SB + e;
        if (i >= n) break;
        const double u = (x[i * V] - q.mx) / q.l11;
        const double v = ((y[i * V] - q.my) - q.l21 * u) / q.l22;
        W[p * n + i] = make_double2(u, v);
        ul = fmin(ul, u); uh = fmax(uh, u);
        vl = fmin(vl, v); vh = fmax(vh, v);
    }
    ul = block_max_waveorder(-ul, red);
    uh = block_max_waveorder(uh, red);
    vl = block_max_waveorder(-vl, red);
    vh = block_max_waveorder(vh, red);
    if (threadIdx.x == 0) {
        double *b = box + (p * nblk + blk) * 4;
        b[0] = -ul; b[1] = uh; b[2] = -vl; b[3] = vh;
    }
}

// Z [P, gx gy]: tile blockIdx.x (G TB consecutive grid points, lane-major: point = tile base + g TB + thread) of pair
// blockIdx.y.  grid [P, gx + gy]: the x then the y coordinates.  The samples pass through LDS in blocks of MG_KDE_SB and
// are read as wavefront-uniform broadcasts; every lane keeps G accumulators, one per grid point of its own.  Two shapes:
// wide (G = 4, TB = 256: independent work beside each exp's dependent chain) where the tiles fill the device, narrow
// (G = 1, TB = 64) where they would not; a Z has the same bits in both.
template <int G, int TB>
__global__ void __launch_bounds__(TB) k_pair_kde2d(int64_t n, const KdePair *par, const double2 *W, const double *box,
                                                     int64_t nblk, const double *grid, int gx, int gy, int skip, double *Z)
{
#pragma clang fp contract(off)
    __shared__ double2 sw[MG_KDE_SB];
    __shared__ double red[TB / 64];
    const int64_t p = blockIdx.y;
    const KdePair q = par[p];
    const int64_t npt = (int64_t)gx * gy, base = (int64_t)blockIdx.x * (G * TB);
    double *z = Z + p * npt;
    if (!q.ok) {
        for (int g = 0; g < G; g++) {
            const int64_t pt = base + (int64_t)g * TB + threadIdx.x;
            if (pt < npt) z[pt] = __builtin_nan("");
        }
        return;
    }
    const double *cx = grid + p * (gx + gy), *cy = cx + gx;
    double gu[G], gv[G], acc[G];
    double ul = MG_INF, uh = -MG_INF, vl = MG_INF, vh = -MG_INF;
#pragma unroll
    for (int g = 0; g < G; g++) {
        int64_t pt = base + (int64_t)g * TB + threadIdx.x;
        if (pt >= npt) pt = npt - 1;   // a spare lane repeats the last point and stores nothing
        const double u = (cx[pt / gy] - q.mx) / q.l11;
        gu[g] = u;
        gv[g] = ((cy[pt % gy] - q.my) - q.l21 * u) / q.l22;
        acc[g] = 0.0;
        ul = fmin(ul, u); uh = fmax(uh, u);
        vl = fmin(vl, gv[g]); vh = fmax(vh, gv[g]);
    }
    // the tile's bounding box in whitened coordinates, the same bits in every thread
    ul = -block_max_waveorder(-ul, red);
    uh = block_max_waveorder(uh, red);
    vl = -block_max_waveorder(-vl, red);
    vh = block_max_waveorder(vh, red);
    const double2 *w = W + p * n;
    const double *bx = box + p * nblk * 4;
    for (int64_t blk = 0; blk < nblk; blk++) {
        if (skip) {
            // the smallest distance between the two boxes bounds every arg of the block from below (workgroup-uniform)
            const double *b = bx + blk * 4;
            const double du = fmax(fmax(ul - b[1], b[0] - uh), 0.0), dv = fmax(fmax(vl - b[3], b[2] - vh), 0.0);
            if (0.5 * (du * du + dv * dv) > MG_KDE_SKIP) continue;
        }
        const int64_t s0 = blk * MG_KDE_SB;
        const int cnt = (int)(n - s0 < MG_KDE_SB ? n - s0 : MG_KDE_SB);
        __syncthreads();   // the previous block has been read
        for (int e = threadIdx.x; e < cnt; e += TB) sw[e] = w[s0 + e];
        __syncthreads();
        for (int e = 0; e < cnt; e++) {
            const double2 s = sw[e];
#pragma unroll
            for (int g = 0; g < G; g++) {
                const double du = gu[g] - s.x, dv = gv[g] - s.y;
                const double arg = du * du + dv * dv;
                acc[g] += exp(-arg / 2.0);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
        const int64_t pt = base + (int64_t)g * TB + threadIdx.x;
        if (pt < npt) z[pt] = acc[g] * q.scale;
    }
}

// ---------------------------------------------------------------------------------------------- spherical KDE
// U [n, 3] = (sin t cos p, sin t sin p, cos t) with, transform != 0 (vonmises_fisher, distributions.py:289-296),
// t = deg2rad(90 - lat), p = deg2rad(mod(lon, 360)); transform == 0 (vonmises_std, :327): t = deg2rad(lat), p = deg2rad(lon)
__global__ void __launch_bounds__(MG_TB) k_sph_unit(int64_t n, const double *lat, const double *lon, int transform, double *U)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * MG_TB + threadIdx.x;
    if (i >= n) return;
    double la = lat[i], lo = lon[i];
    if (transform) {
        la = 90.0 - la;
        lo = fmod(lo, 360.0);
        if (lo < 0.0) lo += 360.0;   // numpy.mod: the sign of the divisor
    }
    const double t = la * (M_PI / 180.0), p = lo * (M_PI / 180.0);
    double st, ct, sp, cp;
    sincos(t, &st, &ct);
    sincos(p, &sp, &cp);
    U[3 * i] = st * cp;
    U[3 * i + 1] = st * sp;
    U[3 * i + 2] = ct;
}

// S [3] = the sum of the rows of U [n, 3]: thread t adds rows t, t + MG_TB, ... ascending, then block_sum_ldstree
__global__ void __launch_bounds__(MG_TB) k_sph_sum(int64_t n, const double *U, double *S)
{
    __shared__ double red[MG_TB];
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < n; i += MG_TB)
        for (int c = 0; c < 3; c++) s[c] += U[3 * i + c];
    for (int c = 0; c < 3; c++) {
        const double v = block_sum_ldstree<MG_TB>(s[c], red);
        if (threadIdx.x == 0) S[c] = v;
    }
}

// kde [m] = sum_i exp(norm + (x . x0_i) / sigma2) over the samples U0 [n, 3] at the grid vectors Ug [m, 3]: the loop of
// k_pair_kde2d, and its two shapes, with the von Mises-Fisher energy; one accumulator per grid point, samples in ascending
// order
template <int G, int TB>
__global__ void __launch_bounds__(TB) k_sph_kde(int64_t n, const double *U0, int64_t m, const double *Ug, double norm,
                                                  double sigma2, double *kde)
{
#pragma clang fp contract(off)
    __shared__ double sx[MG_KDE_SB], sy[MG_KDE_SB], sz[MG_KDE_SB];
    const int64_t base = (int64_t)blockIdx.x * (G * TB);
    double gx[G], gy[G], gz[G], acc[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        int64_t pt = base + (int64_t)g * TB + threadIdx.x;
        if (pt >= m) pt = m - 1;
        gx[g] = Ug[3 * pt];
        gy[g] = Ug[3 * pt + 1];
        gz[g] = Ug[3 * pt + 2];
        acc[g] = 0.0;
    }
    for (int64_t s0 = 0; s0 < n; s0 += MG_KDE_SB) {
        const int cnt = (int)(n - s0 < MG_KDE_SB ? n - s0 : MG_KDE_SB);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt; e += TB) {
            sx[e] = U0[3 * (s0 + e)];
            sy[e] = U0[3 * (s0 + e) + 1];
            sz[e] = U0[3 * (s0 + e) + 2];
        }
        __syncthreads();
        for (int e = 0; e < cnt; e++) {
            const double x0 = sx[e], y0 = sy[e], z0 = sz[e];
#pragma unroll
            for (int g = 0; g < G; g++) {
                const double dot = (gx[g] * x0 + gy[g] * y0) + gz[g] * z0;
                acc[g] += exp(norm + dot / sigma2);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
        const int64_t pt = base + (int64_t)g * TB + threadIdx.x;
        if (pt < m) kde[pt] = acc[g];
    }
}

}  // namespace

// ================================================================================================ launchers
int launch_col_check(beatamd_ctx *ctx, const double *X, int64_t n, int64_t V, const int64_t *cols, int64_t K, int32_t *flags)
{
    if (K == 0 || n == 0) return BEATAMD_OK;
    BA_CHECK(K <= 65535, BEATAMD_EINVAL, "marginals: more than 65535 columns in one call");
    BA_HIP(hipMemsetAsync(flags, 0, (size_t)K * sizeof(int32_t), ctx->stream));
    const int64_t nb = std::min<int64_t>((n + MG_TB - 1) / MG_TB, 64);
    hipLaunchKernelGGL(k_col_check, dim3((unsigned)nb, (unsigned)K), dim3(MG_TB), 0, ctx->stream, X, n, V, cols, flags);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

static int64_t mg_pow2(int64_t n)
{
    int64_t p = 2;
    while (p < n) p <<= 1;
    return p;
}

int launch_col_sort(beatamd_ctx *ctx, const double *X, int64_t n, int64_t V, const int64_t *cols, int64_t K, double *out)
{
    if (K == 0 || n == 0) return BEATAMD_OK;
    BA_CHECK(K <= 65535, BEATAMD_EINVAL, "column_sort: more than 65535 columns in one call");
    BA_CHECK(n <= MG_SORT_MAX_N, BEATAMD_EINVAL, "column_sort: %lld samples, at most %lld", (long long)n, (long long)MG_SORT_MAX_N);
    ScopedTimer tm(ctx, "col_sort");
    const int64_t npad = mg_pow2(n);
    const int L = (int)std::min<int64_t>(npad, MG_SORT_TILE);
    const int64_t ntile = npad / L;
    const size_t lds = (size_t)L * sizeof(double);
    BA_HIP(hipFuncSetAttribute((const void *)k_col_sort_tile, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(MG_SORT_TILE * sizeof(double))));
    const dim3 tg((unsigned)ntile, (unsigned)K), gg((unsigned)((npad / 2 + MG_TB - 1) / MG_TB), (unsigned)K);
    hipLaunchKernelGGL(k_col_sort_tile, tg, dim3(MG_SORT_TB), lds, ctx->stream, X, n, V, cols, out, L, 0);
    for (int64_t kk = 2 * (int64_t)L; kk <= npad; kk <<= 1) {
        hipLaunchKernelGGL(k_col_sort_global, gg, dim3(MG_TB), 0, ctx->stream, out, n, npad, kk / 2, 1);
        for (int64_t s = kk / 4; s >= L; s >>= 1)
            hipLaunchKernelGGL(k_col_sort_global, gg, dim3(MG_TB), 0, ctx->stream, out, n, npad, s, 0);
        hipLaunchKernelGGL(k_col_sort_tile, tg, dim3(MG_SORT_TB), lds, ctx->stream, X, n, V, cols, out, L, 1);
    }
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_col_percentiles(beatamd_ctx *ctx, const double *S, int64_t K, int64_t n, const double *q, int64_t Q, double *out)
{
    if (K * Q == 0) return BEATAMD_OK;
    const int64_t nb = (K * Q + MG_TB - 1) / MG_TB;
    BA_CHECK(nb < (int64_t)0x7fffffff, BEATAMD_EINVAL, "column_percentiles: too many results");
    hipLaunchKernelGGL(k_col_percentiles, dim3((unsigned)nb), dim3(MG_TB), 0, ctx->stream, S, K, n, q, Q, out);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_col_hist(beatamd_ctx *ctx, const double *S, int64_t K, int64_t n, const double *edges, int64_t nb, int64_t *counts)
{
    if (K == 0 || nb == 0) return BEATAMD_OK;
    BA_CHECK(K <= 65535, BEATAMD_EINVAL, "column_histograms: more than 65535 columns in one call");
    hipLaunchKernelGGL(k_col_hist, dim3((unsigned)((nb + MG_TB - 1) / MG_TB), (unsigned)K), dim3(MG_TB), 0, ctx->stream, S, n,
                       edges, nb, counts);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_pair_hist2d(beatamd_ctx *ctx, const double *X, int64_t n, int64_t V, const int64_t *pairs, int64_t P, int bx, int by,
                       const double *xedges, const double *yedges, int64_t *counts)
{
    if (P == 0) return BEATAMD_OK;
    BA_CHECK(P < (int64_t)0x7fffffff && n < ((int64_t)1 << 32), BEATAMD_EINVAL, "pair_hist2d: batch too large");
    ScopedTimer tm(ctx, "pair_hist2d");
    BA_HIP(hipMemsetAsync(counts, 0, (size_t)P * bx * by * sizeof(int64_t), ctx->stream));
    if (n == 0) return BEATAMD_OK;
    const size_t lds = (size_t)(bx + 1 + by + 1) * sizeof(double) + (size_t)bx * by * sizeof(uint32_t);
    BA_HIP(hipFuncSetAttribute((const void *)k_pair_hist2d, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)((2 * MG_HIST2D_MAX_SIDE + 2) * sizeof(double) + MG_HIST2D_MAX_CELLS * sizeof(uint32_t))));
    const int64_t split = std::max<int64_t>(1, std::min<int64_t>(n / 8192, 16));
    hipLaunchKernelGGL(k_pair_hist2d, dim3((unsigned)P, (unsigned)split), dim3(MG_TB), lds, ctx->stream, X, n, V, pairs, bx, by,
                       xedges, yedges, reinterpret_cast<unsigned long long *>(counts));
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_pair_moments(beatamd_ctx *ctx, const double *X, int64_t n, int64_t V, const int64_t *pairs, int64_t P, double *mom)
{
    if (P == 0) return BEATAMD_OK;
    BA_CHECK(P < (int64_t)0x7fffffff, BEATAMD_EINVAL, "pair_moments: batch too large");
    hipLaunchKernelGGL(k_pair_moments, dim3((unsigned)P), dim3(MG_TB), 0, ctx->stream, X, n, V, pairs, mom);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_sph_unit(beatamd_ctx *ctx, int64_t n, const double *lat, const double *lon, int transform, double *U)
{
    if (n == 0) return BEATAMD_OK;
    const int64_t nb = (n + MG_TB - 1) / MG_TB;
    BA_CHECK(nb < (int64_t)0x7fffffff, BEATAMD_EINVAL, "spherical_kde: too many points");
    hipLaunchKernelGGL(k_sph_unit, dim3((unsigned)nb), dim3(MG_TB), 0, ctx->stream, n, lat, lon, transform, U);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_sph_sum(beatamd_ctx *ctx, int64_t n, const double *U, double *S)
{
    hipLaunchKernelGGL(k_sph_sum, dim3(1), dim3(MG_TB), 0, ctx->stream, n, U, S);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// wide where its tiles give every compute unit two workgroups, narrow below; shape 1 / 2 force wide / narrow
static bool kde_wide(int shape, int64_t points, int64_t P)
{
    return shape == 1 || (shape != 2 && (points + MG_KDE_TILE - 1) / MG_KDE_TILE * P >= 512);
}

int launch_sph_kde(beatamd_ctx *ctx, int64_t n, const double *U0, int64_t m, const double *Ug, double norm, double sigma2,
                   int shape, double *kde)
{
    if (m == 0) return BEATAMD_OK;
    const bool wide = kde_wide(shape, m, 1);
    const int64_t tile = wide ? MG_KDE_TILE : 64, ntile = (m + tile - 1) / tile;
    BA_CHECK(ntile < (int64_t)0x7fffffff, BEATAMD_EINVAL, "spherical_kde: grid too large");
    ScopedTimer tm(ctx, "sph_kde");
    if (wide)
        hipLaunchKernelGGL((k_sph_kde<MG_KDE_G, MG_TB>), dim3((unsigned)ntile), dim3(MG_TB), 0, ctx->stream, n, U0, m, Ug, norm,
                           sigma2, kde);
    else
        hipLaunchKernelGGL((k_sph_kde<1, 64>), dim3((unsigned)ntile), dim3(64), 0, ctx->stream, n, U0, m, Ug, norm, sigma2, kde);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_pair_kde2d(beatamd_ctx *ctx, const double *X, int64_t n, int64_t V, const int64_t *pairs, int64_t P,
                      const KdePair *par, double *W, double *box, const double *grid, int gx, int gy, int skip, int shape,
                      double *Z)
{
    if (P == 0) return BEATAMD_OK;
    const bool wide = kde_wide(shape, (int64_t)gx * gy, P);
    const int64_t tile = wide ? MG_KDE_TILE : 64;
    const int64_t nblk = kde_sample_blocks(n), ntile = ((int64_t)gx * gy + tile - 1) / tile;
    BA_CHECK(P <= 65535 && nblk < (int64_t)0x7fffffff && ntile < (int64_t)0x7fffffff, BEATAMD_EINVAL,
             "pair_kde2d: batch too large");
    ScopedTimer tm(ctx, "pair_kde2d");
    hipLaunchKernelGGL(k_pair_whiten, dim3((unsigned)nblk, (unsigned)P), dim3(MG_TB), 0, ctx->stream, X, n, V, pairs, par,
                       reinterpret_cast<double2 *>(W), box);
    if (wide)
        hipLaunchKernelGGL((k_pair_kde2d<MG_KDE_G, MG_TB>), dim3((unsigned)ntile, (unsigned)P), dim3(MG_TB), 0, ctx->stream, n,
                           par, reinterpret_cast<const double2 *>(W), box, nblk, grid, gx, gy, skip, Z);
    else
        hipLaunchKernelGGL((k_pair_kde2d<1, 64>), dim3((unsigned)ntile, (unsigned)P), dim3(64), 0, ctx->stream, n, par,
                           reinterpret_cast<const double2 *>(W), box, nblk, grid, gx, gy, skip, Z);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
