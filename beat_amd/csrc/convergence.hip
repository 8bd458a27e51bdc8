// convergence.hip -- the convergence summary of a trace X [C, D, V] (C chains, D draws, V scalar variables, row-major): what
// ``beat summarize`` writes to summary.txt through ``arviz.summary`` (apps/beat.py:1338-1363, backend.py:1401-1415): mean, sd,
// highest-density interval, the bulk / tail / mean / sd effective sample sizes and the rank-normalised split R-hat of every
// variable.  The statistics are restated from memory of arviz's stats/diagnostics.py and of Vehtari et al. (2021),
// unverified against an installed arviz; tests/convergence_ref.py is the numpy restatement of this file.
//
// What the kernels promise:
//   SUMS        every mean and centred sum of squares here (a whole column, a row of a transform) has ONE order: thread t of
//               256 adds the elements t, t + 256, ... ascending, then block_sum_ldstree<256>; the centred sum is a second
//               pass over (x - mean)^2 in the same order.  Sums over the M rows of a row set (mean of the autocovariances,
//               mean and variance of the row means, mean of the row variances) are sequential over ascending m.
//   k_conv_hdi  first minimum of s[j + inc] - s[j] on the sorted column: ties go to the smaller j, so the order is free
//   k_conv_rank_z   average rank = (lower bound + upper bound + 1) / 2 from two binary searches in the sorted values (-0.0
//               and 0.0 tie), then normcdfinv((r - 3/8) / (n + 1/4))
//   k_acov_lags acov[k] = (sum over the chunks c = 0, 1, ... of CV_ACOV_CHUNK consecutive i, ascending, of the chunk's sum
//               over ascending i of (y_i - m)(y_{i+k} - m), ONE accumulator per lag that starts from 0.0, product then sum, not
//               contracted) / n.  Terms with i + k >= n are exact zeros.  A lag's value depends neither on the lag block
//               nor on the lags per lane, the rows, the round that computed it or the workgroups its chunks were dealt to
//               (every chunk sum is stored; k_acov_combine adds them in order).
//   k_conv_geyer    Geyer's initial monotone sequence as arviz's _ess loop runs it, on the lags at hand: an ESS, or "needs
//               more lags"; the sum of the rho is sequential ascending
// No floating-point atomics, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "ctx.hpp"
#include "devmath.hpp"
#include "kernels.hpp"
#include "wave.hpp"

namespace beatamd {

namespace {

constexpr int CV_TB = 256;
constexpr double CV_INF = __builtin_huge_val();
constexpr double CV_NAN = __builtin_nan("");

// element j of row m of split(X[:, :, col]): rows 0 .. C - 1 the first h draws of the chains, C .. 2C - 1 their last h
__device__ __forceinline__ int64_t cv_split_index(int64_t m, int64_t j, int64_t C, int64_t D, int64_t h, int64_t V)
{
    const int64_t c = m < C ? m : m - C, d = m < C ? j : D - h + j;
    return (c * D + d) * V;
}

// out[k] = base + k * step
__global__ void __launch_bounds__(CV_TB) k_conv_iota(int64_t *out, int64_t K, int64_t base, int64_t step)
{
    const int64_t k = (int64_t)blockIdx.x * CV_TB + threadIdx.x;
    if (k < K) out[k] = base + k * step;
}

// ---------------------------------------------------------------------------------------------- moments
// mom [R, 4] = (mean, centred sum of squares, min, max) of the R series x_r[i] = base[off(r) + i * stride], i < n; the
// SUMS order.  off == nullptr: row r starts at r * n * stride.
__global__ void __launch_bounds__(CV_TB) k_conv_moments(const double *base, const int64_t *off, int64_t n, int64_t stride,
                                                       double *mom)
{
#pragma clang fp contract(off)
    __shared__ double red[CV_TB];
    const int64_t r = blockIdx.x;
    const double *x = base + (off ? off[r] : r * n * stride);
    double s = 0.0, lo = CV_INF, hi = -CV_INF;
    for (int64_t i = threadIdx.x; i < n; i += CV_TB) {
        const double a = x[i * stride];
        s += a;
        lo = fmin(lo, a);
        hi = fmax(hi, a);
    }
    const double mean = block_sum_ldstree<CV_TB>(s, red) / (double)n;
    double q = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += CV_TB) {
        const double a = x[i * stride] - mean;
        q += a * a;
    }
    q = block_sum_ldstree<CV_TB>(q, red);
    lo = block_max_waveorder(-lo, red);   // min = -max(-x): exact
    hi = block_max_waveorder(hi, red);
    if (threadIdx.x == 0) {
        double *m = mom + r * 4;
        m[0] = mean; m[1] = q; m[2] = -lo; m[3] = hi;
    }
}

// ---------------------------------------------------------------------------------------------- HDI
// hdi [K, 2] = (s[j], s[j + inc]) with j the first minimum of s[j + inc] - s[j], j < n - inc, on the sorted rows S [K, n]
__global__ void __launch_bounds__(CV_TB) k_conv_hdi(const double *S, int64_t n, int64_t inc, double *hdi)
{
#pragma clang fp contract(off)
    __shared__ double wv[CV_TB];
    __shared__ int64_t wj[CV_TB];
    const double *s = S + (int64_t)blockIdx.x * n;
    double best = CV_INF;
    int64_t bj = n;   // n: nothing found (a NaN column)
    for (int64_t j = threadIdx.x; j < n - inc; j += CV_TB) {
        const double w = s[j + inc] - s[j];
        if (w < best || (w == best && j < bj)) {
            best = w;
            bj = j;
        }
    }
    wv[threadIdx.x] = best;
    wj[threadIdx.x] = bj;
    __syncthreads();
    for (int hh = CV_TB / 2; hh > 0; hh >>= 1) {
        if ((int)threadIdx.x < hh) {
            const double w = wv[threadIdx.x + hh];
            const int64_t j = wj[threadIdx.x + hh];
            if (w < wv[threadIdx.x] || (w == wv[threadIdx.x] && j < wj[threadIdx.x])) {
                wv[threadIdx.x] = w;
                wj[threadIdx.x] = j;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int64_t j = wj[0];
        hdi[2 * blockIdx.x] = j < n ? s[j] : CV_NAN;
        hdi[2 * blockIdx.x + 1] = j < n ? s[j + inc] : CV_NAN;
    }
}

// ---------------------------------------------------------------------------------------------- transforms
// W [K, 6, M, h]: row set 0 = split(X[:, :, cols[k]])
__global__ void __launch_bounds__(CV_TB) k_conv_write_raw(const double *X, int64_t C, int64_t D, int64_t V, const int64_t *cols,
                                                         int64_t h, double *W)
{
    const int64_t n2 = 2 * C * h, e = (int64_t)blockIdx.x * CV_TB + threadIdx.x, k = blockIdx.y;
    if (e >= n2) return;
    W[k * CV_NT * n2 + e] = X[cols[k] + cv_split_index(e / h, e % h, C, D, h, V)];
}

// row sets 1, 2, 3 and, unranked, 5 from row set 0: (x - mean)^2, x <= q05, x <= q95, |x - median of the split values|
// cm [K, 4]: the column's moments; qa [K, 2]: its 5 % and 95 % quantiles; med [K]
__global__ void __launch_bounds__(CV_TB) k_conv_write_derived(double *W, int64_t n2, const double *cm, const double *qa,
                                                             const double *med)
{
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * CV_TB + threadIdx.x, k = blockIdx.y;
    if (e >= n2) return;
    double *w = W + k * CV_NT * n2;
    const double x = w[e], d = x - cm[4 * k];
    w[n2 + e] = d * d;
    w[2 * n2 + e] = x <= qa[2 * k] ? 1.0 : 0.0;
    w[3 * n2 + e] = x <= qa[2 * k + 1] ? 1.0 : 0.0;
    w[5 * n2 + e] = fabs(x - med[k]);
}

// z[e] = normcdfinv((rank - 3/8) / (n + 1/4)) of vals[e] among the sorted values of its set; set k: vals + k * vstride [n],
// sorted S + k * n, z + k * zstride (z may be vals: every element is read once, by the thread that writes it);
// ranks != nullptr: the average ranks [K, n] as well
__global__ void __launch_bounds__(CV_TB) k_conv_rank_z(const double *vals, int64_t vstride, const double *S, int64_t n, double *z,
                                                      int64_t zstride, double *ranks)
{
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * CV_TB + threadIdx.x, k = blockIdx.y;
    if (e >= n) return;
    const double x = vals[k * vstride + e];
    const double *s = S + k * n;
    const int64_t lo = sorted_bound(s, n, x, false), hi = sorted_bound(s, n, x, true);
    const double r = (double)(lo + hi + 1) / 2.0;   // the mean of the ranks lo + 1 .. hi
    if (ranks) ranks[k * n + e] = r;
    z[k * zstride + e] = normcdfinv((r - 0.375) / ((double)n + 0.25));
}

// ---------------------------------------------------------------------------------------------- lagged products
// part [nrow, nchunk, nlags]: the chunk sums; row x of the launch is series rows[x / M] * M + x % M of Y [., n] (rows ==
// nullptr: series x), centred by mom[4 * series]; lag k = lag0 + (blockIdx.y * 64 + lane) * L + j, j < L; workgroup z takes
// the chunks z cpb .. (z + 1) cpb, each into an accumulator of its own.  One wavefront a workgroup.  Per chunk and
// tile the centred values y[i0 .. i0 + T) (read by all lanes at once) and y[i0 + kb .. i0 + kb + T + 64 L) (the lag side)
// stand in LDS, zero past the end of the series.  A lane keeps L accumulators, one per lag of its own, and a window of the
// lag side in registers that moves by four per step: sixteen (L = 4) products for four reads of two doubles.
template <int L>
__global__ void __launch_bounds__(64) k_acov_lags(const double *Y, const double *mom, const int32_t *rows, int64_t M, int64_t n,
                                                  int64_t lag0, int64_t nlags, int64_t cpb, double *part)
{
#pragma clang fp contract(off)
    constexpr int T = CV_ACOV_TILE, HB = T + 64 * L;
    __shared__ __attribute__((aligned(16))) double sa[T];
    __shared__ __attribute__((aligned(16))) double sb[HB];
    const int lane = threadIdx.x;
    const int64_t x = blockIdx.x, series = rows ? (int64_t)rows[x / M] * M + x % M : x;
    const double *y = Y + series * n;
    const double mean = mom[4 * series];
    const int64_t kb = lag0 + (int64_t)blockIdx.y * 64 * L;
    const int b = lane * L;
    const int64_t nchunk = (n + CV_ACOV_CHUNK - 1) / CV_ACOV_CHUNK, cfirst = (int64_t)blockIdx.z * cpb;
    const int64_t clast = cfirst + cpb < nchunk ? cfirst + cpb : nchunk;
    for (int64_t c = cfirst; c < clast; c++) {
        const int64_t c0 = c * CV_ACOV_CHUNK;
        double acc[L];
#pragma unroll
        for (int j = 0; j < L; j++) acc[j] = 0.0;
        const int64_t c1 = c0 + CV_ACOV_CHUNK < n ? c0 + CV_ACOV_CHUNK : n;
        for (int64_t i0 = c0; i0 < c1; i0 += T) {
            __syncthreads();   // the previous tile has been read
            for (int t = lane; t < T; t += 64) sa[t] = i0 + t < n ? y[i0 + t] - mean : 0.0;
            for (int t = lane; t < HB; t += 64) {
                const int64_t i = i0 + kb + t;
                sb[t] = i < n ? y[i] - mean : 0.0;
            }
            __syncthreads();
            if (L == 1) {
                for (int t = 0; t < T; t += 4) {
#pragma unroll
                    for (int s = 0; s < 4; s++) acc[0] += sa[t + s] * sb[t + s + b];
                }
            } else {
                double w[L + 4];
#pragma unroll
                for (int j = 0; j < L; j++) w[j] = sb[b + j];
                for (int t = 0; t < T; t += 4) {
                    double a[4];
#pragma unroll
                    for (int s = 0; s < 4; s++) {
                        a[s] = sa[t + s];
                        w[L + s] = sb[t + b + L + s];
                    }
#pragma unroll
                    for (int s = 0; s < 4; s++)
#pragma unroll
                        for (int j = 0; j < L; j++) acc[j] += a[s] * w[s + j];
#pragma unroll
                    for (int j = 0; j < L; j++) w[j] = w[j + 4];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < L; j++) {
            const int64_t k = (int64_t)blockIdx.y * 64 * L + b + j;
            if (k < nlags) part[(x * nchunk + c) * nlags + k] = acc[j];
        }
    }
}

// out [nrow, ldo] columns o0 .. o0 + nlags = (the chunk sums part [nrow, nchunk, nlags] added in ascending order from 0.0) / n
__global__ void __launch_bounds__(CV_TB) k_acov_combine(const double *part, int64_t nchunk, int64_t nlags, int64_t n, double *out,
                                                       int64_t ldo, int64_t o0)
{
#pragma clang fp contract(off)
    const int64_t k = (int64_t)blockIdx.x * CV_TB + threadIdx.x, x = blockIdx.y;
    if (k >= nlags) return;
    double tot = 0.0;
    for (int64_t c = 0; c < nchunk; c++) tot += part[(x * nchunk + c) * nlags + k];
    out[x * ldo + o0 + k] = tot / (double)n;
}

// mac [A, ld] columns l0 .. l0 + nl: the mean over the M rows (sequential, ascending m) of ac [A * M, nl]
__global__ void __launch_bounds__(CV_TB) k_conv_lagmean(const double *ac, int64_t M, int64_t nl, double *mac, int64_t ld, int64_t l0)
{
#pragma clang fp contract(off)
    const int64_t k = (int64_t)blockIdx.x * CV_TB + threadIdx.x, a = blockIdx.y;
    if (k >= nl) return;
    double s = 0.0;
    for (int64_t m = 0; m < M; m++) s += ac[(a * M + m) * nl + k];
    mac[a * ld + l0 + k] = s / (double)M;
}

// dst [A2, ld2] columns 0 .. nl = the rows src_row[a] of src [., ld]
__global__ void __launch_bounds__(CV_TB) k_conv_regroup(const double *src, int64_t ld, const int32_t *src_row, int64_t nl,
                                                       double *dst, int64_t ld2)
{
    const int64_t k = (int64_t)blockIdx.x * CV_TB + threadIdx.x, a = blockIdx.y;
    if (k < nl) dst[a * ld2 + k] = src[(int64_t)src_row[a] * ld + k];
}

// ---------------------------------------------------------------------------------------------- Geyer's sequence
// One lane per active group a (row set groups[a] of M rows of n values, row moments rm [., 4]): arviz's _ess on the lags
// mac [a, 0 .. avail) at hand.  state[a] = 0 and ess[groups[a]] set, or state[a] = 1: the scan wants a lag >= avail.
// rho [A, ld]: work space.  tau_floor = 1 / log10(M n).
__global__ void __launch_bounds__(64) k_conv_geyer(int64_t A, const int32_t *groups, int64_t M, int64_t n, const double *rm,
                                                   const double *mac, double *rho_ws, int64_t ld, int64_t avail, double tau_floor,
                                                   double *ess, int32_t *state)
{
#pragma clang fp contract(off)
    const int64_t a = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (a >= A) return;
    const int64_t g = groups[a];
    const double *r = rm + g * M * 4, *ac = mac + a * ld;
    double *rho = rho_ws + a * ld;
    const double dn = (double)n, size = (double)(M * n);
    state[a] = 0;
    double lo = r[2], hi = r[3];
    for (int64_t m = 1; m < M; m++) {
        lo = fmin(lo, r[4 * m + 2]);
        hi = fmax(hi, r[4 * m + 3]);
    }
    if (hi - lo < 1e-15) {
        ess[g] = size;
        return;
    }
    const double mean_var = ac[0] * dn / (dn - 1.0);
    double var_plus = mean_var * (dn - 1.0) / dn;
    if (M > 1) {
        double s = 0.0;
        for (int64_t m = 0; m < M; m++) s += r[4 * m];
        const double mm = s / (double)M;
        double q = 0.0;
        for (int64_t m = 0; m < M; m++) {
            const double d = r[4 * m] - mm;
            q += d * d;
        }
        var_plus += q / (double)(M - 1);
    }
#define CV_RHO(t) (1.0 - (mean_var - ac[t]) / var_plus)
    bool nan = false;
    double even = 1.0, odd = CV_RHO(1);
    rho[0] = 1.0;
    rho[1] = odd;
    nan = nan || odd != odd;
    int64_t t = 1;
    while (t < n - 3 && even + odd > 0.0) {
        if (t + 2 >= avail) {
            state[a] = 1;
            return;
        }
        even = CV_RHO(t + 1);
        odd = CV_RHO(t + 2);
        const bool keep = even + odd >= 0.0;
        rho[t + 1] = keep ? even : 0.0;
        rho[t + 2] = keep ? odd : 0.0;
        nan = nan || (keep && (even != even || odd != odd));
        t += 2;
    }
#undef CV_RHO
    const int64_t max_t = t - 2;
    if (even > 0.0) rho[max_t + 1] = even;
    for (int64_t u = 1; u <= max_t - 2; u += 2)
        if (rho[u + 1] + rho[u + 2] > rho[u - 1] + rho[u]) {
            const double v = (rho[u - 1] + rho[u]) / 2.0;
            rho[u + 1] = v;
            rho[u + 2] = v;
        }
    double s = 0.0;
    for (int64_t u = 0; u <= max_t; u++) s += rho[u];
    double tau = (-1.0 + 2.0 * s) + rho[max_t + 1];
    if (!(tau >= tau_floor)) tau = tau == tau ? tau_floor : tau;   // max(tau, floor); a NaN stays
    ess[g] = nan ? CV_NAN : size / tau;
}

// rhat [K] = max over the row sets 4 and 5 of sqrt((B / W + n - 1) / n), B = n var(row means, ddof 1), W = mean(row variances)
__global__ void __launch_bounds__(64) k_conv_rhat(int64_t K, int64_t M, int64_t n, const double *rm, double *rhat)
{
#pragma clang fp contract(off)
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    const double dn = (double)n;
    double best = 0.0;
    bool nan = false;
    for (int set = 4; set < 6; set++) {
        const double *r = rm + (k * CV_NT + set) * M * 4;
        double s = 0.0, w = 0.0;
        for (int64_t m = 0; m < M; m++) {
            s += r[4 * m];
            w += r[4 * m + 1] / (dn - 1.0);
        }
        const double mm = s / (double)M;
        double q = 0.0;
        for (int64_t m = 0; m < M; m++) {
            const double d = r[4 * m] - mm;
            q += d * d;
        }
        const double B = dn * (q / (double)(M - 1)), W = w / (double)M;
        const double v = sqrt(((B / W + dn) - 1.0) / dn);
        nan = nan || v != v;
        best = fmax(best, v);
    }
    rhat[k] = nan ? CV_NAN : best;
}

// out [K, 11] = mean, sd, hdi_lo, hdi_hi, NaN, NaN (the two MCSE: formed by the caller), ess_bulk, ess_tail, r_hat, ess_mean,
// ess_sd; diag == 0: no diagnostics (fewer than 4 draws); a flagged column is all NaN
__global__ void __launch_bounds__(CV_TB) k_conv_finish(int64_t K, int64_t S, const double *cm, const double *hdi, const double *ess,
                                                      const double *rhat, const int32_t *flags, int diag, double *out)
{
#pragma clang fp contract(off)
    const int64_t k = (int64_t)blockIdx.x * CV_TB + threadIdx.x;
    if (k >= K) return;
    double *o = out + k * CV_NCOL;
    for (int c = 0; c < CV_NCOL; c++) o[c] = CV_NAN;
    if (flags[k]) return;
    o[0] = cm[4 * k];
    o[1] = sqrt(cm[4 * k + 1] / (double)(S - 1));
    o[2] = hdi[2 * k];
    o[3] = hdi[2 * k + 1];
    if (!diag) return;
    const double *e = ess + k * CV_NT;
    o[6] = e[4];
    o[7] = (e[2] != e[2] || e[3] != e[3]) ? CV_NAN : fmin(e[2], e[3]);
    o[8] = rhat[k];
    o[9] = e[0];
    o[10] = e[1];
}

inline unsigned cv_blocks(int64_t n) { return (unsigned)((n + CV_TB - 1) / CV_TB); }

// out [nrow, nlags].  The lags go in ranges that keep the chunk sums within CV_PART_BYTES, the chunks of a range over as
// many workgroups as fill the device: neither changes a bit (every chunk has its own sum, added in order by k_acov_combine).
int cv_lags(beatamd_ctx *ctx, const double *Y, const double *mom, const int32_t *rows, int64_t nrow, int64_t M, int64_t n,
            int64_t lag0, int64_t nlags, double *out)
{
    if (nrow == 0 || nlags == 0) return BEATAMD_OK;
    BA_CHECK(nrow < (int64_t)0x7fffffff, BEATAMD_EINVAL, "autocov_lags: %lld rows in one launch", (long long)nrow);
    ScopedTimer tm(ctx, "acov_lags");
    const int64_t nchunk = (n + CV_ACOV_CHUNK - 1) / CV_ACOV_CHUNK;
    const int64_t fit = CV_PART_BYTES / (int64_t)sizeof(double) / std::max<int64_t>(1, nrow * nchunk);
    const int64_t range = std::min<int64_t>(nlags, std::max<int64_t>(256, fit / 256 * 256));
    double *d_part;
    BA_TRY(ctx->scratch(SL_CV_PART, (size_t)(nrow * nchunk * range), &d_part));
    for (int64_t r0 = 0; r0 < nlags; r0 += range) {
        const int64_t nl = std::min(range, nlags - r0);
        const int L = nl <= 64 ? 1 : 4;
        const int64_t nb = (nl + 64 * L - 1) / (64 * L);
        // chunks a workgroup: about four wavefronts a SIMD over the device, at most 65535 workgroups along z
        const int64_t cpb = std::max<int64_t>(std::min<int64_t>(nchunk, nrow * nb * nchunk / (16 * (int64_t)ctx->num_cu)),
                                              (nchunk + 65534) / 65535);
        const int64_t nz = (nchunk + std::max<int64_t>(cpb, 1) - 1) / std::max<int64_t>(cpb, 1);
        BA_CHECK(nb <= 65535, BEATAMD_EINVAL, "autocov_lags: %lld lags in one launch", (long long)nl);
        const dim3 grid((unsigned)nrow, (unsigned)nb, (unsigned)nz);
        if (L == 1)
            hipLaunchKernelGGL((k_acov_lags<1>), grid, dim3(64), 0, ctx->stream, Y, mom, rows, M, n, lag0 + r0, nl,
                               std::max<int64_t>(cpb, 1), d_part);
        else
            hipLaunchKernelGGL((k_acov_lags<4>), grid, dim3(64), 0, ctx->stream, Y, mom, rows, M, n, lag0 + r0, nl,
                               std::max<int64_t>(cpb, 1), d_part);
        for (int64_t x0 = 0; x0 < nrow; x0 += 65535) {
            const int64_t nx = std::min<int64_t>(65535, nrow - x0);
            hipLaunchKernelGGL(k_acov_combine, dim3(cv_blocks(nl), (unsigned)nx), dim3(CV_TB), 0, ctx->stream,
                               d_part + x0 * nchunk * nl, nchunk, nl, n, out + x0 * nlags, nlags, r0);
        }
        BA_HIP(hipGetLastError());
    }
    return BEATAMD_OK;
}

template <class T>
int cv_readback(beatamd_ctx *ctx, const T *d, size_t n, std::vector<T> &h)
{
    h.resize(n);
    BA_HIP(hipMemcpyAsync(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    BA_HIP(hipStreamSynchronize(ctx->stream));
    return BEATAMD_OK;
}

}  // namespace

// ================================================================================================ launchers
int launch_autocov_lags(beatamd_ctx *ctx, int64_t R, int64_t n, const double *Y, int64_t lag0, int64_t nlags, double *out)
{
    if (R == 0 || nlags == 0) return BEATAMD_OK;
    BA_CHECK(R < (int64_t)0x7fffffff, BEATAMD_EINVAL, "autocov_lags: too many rows");
    double *d_mom;
    BA_TRY(ctx->scratch(SL_CV_RM, (size_t)R * 4, &d_mom));
    hipLaunchKernelGGL(k_conv_moments, dim3((unsigned)R), dim3(CV_TB), 0, ctx->stream, Y, (const int64_t *)nullptr, n, (int64_t)1,
                       d_mom);
    BA_HIP(hipGetLastError());
    return cv_lags(ctx, Y, d_mom, nullptr, R, 1, n, lag0, nlags, out);
}

int launch_rank_normalize(beatamd_ctx *ctx, int64_t n, const double *A, double *z, double *ranks)
{
    if (n == 0) return BEATAMD_OK;
    BA_CHECK(n <= MG_SORT_MAX_N, BEATAMD_EINVAL, "rank_normalize: %lld values, at most %lld", (long long)n,
             (long long)MG_SORT_MAX_N);
    double *d_s;
    int64_t *d_off;
    BA_TRY(ctx->scratch(SL_CV_SB, (size_t)n, &d_s));
    BA_TRY(ctx->scratch(SL_CV_OFF, (size_t)1, &d_off));
    hipLaunchKernelGGL(k_conv_iota, dim3(1), dim3(CV_TB), 0, ctx->stream, d_off, (int64_t)1, (int64_t)0, (int64_t)0);
    BA_TRY(launch_col_sort(ctx, A, n, 1, d_off, 1, d_s));
    hipLaunchKernelGGL(k_conv_rank_z, dim3(cv_blocks(n), 1), dim3(CV_TB), 0, ctx->stream, A, (int64_t)0, d_s, n, z, (int64_t)0,
                       ranks);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// one batch of K variables; out [K, CV_NCOL], flags [K] (device)
static int cv_summary_batch(beatamd_ctx *ctx, int64_t C, int64_t D, int64_t V, const double *X, int64_t K, const int64_t *d_cols,
                            int64_t inc, double tau_floor, int64_t first_lags, double *out, int32_t *flags, int64_t *rounds)
{
    const int64_t S = C * D, h = D / 2, M = 2 * C, n2 = M * h;
    const bool diag = D >= 4;
    hipStream_t st = ctx->stream;
    double *d_cm, *d_sa, *d_q, *d_hdi, *d_ess, *d_rhat;
    BA_TRY(ctx->scratch(SL_CV_CM, (size_t)K * 4, &d_cm));
    BA_TRY(ctx->scratch(SL_CV_SA, (size_t)K * std::max(S, n2), &d_sa));
    BA_TRY(ctx->scratch(SL_CV_Q, (size_t)K * 8 + 8, &d_q));   // qa [K, 2], med [K], hdi [K, 2], rhat [K], percents [3]
    BA_TRY(ctx->scratch(SL_CV_ESS, (size_t)K * CV_NT, &d_ess));
    double *d_qa = d_q, *d_med = d_q + 2 * K, *d_pct = d_q + 6 * K;
    d_hdi = d_q + 3 * K;
    d_rhat = d_q + 5 * K;
    const double pct[3] = {5.0, 95.0, 50.0};
    BA_HIP(hipMemcpyAsync(d_pct, pct, sizeof(pct), hipMemcpyHostToDevice, st));
    BA_HIP(hipStreamSynchronize(st));   // (pct lives on this frame)
    BA_TRY(launch_col_check(ctx, X, S, V, d_cols, K, flags));
    hipLaunchKernelGGL(k_conv_moments, dim3((unsigned)K), dim3(CV_TB), 0, st, X, d_cols, S, V, d_cm);
    BA_TRY(launch_col_sort(ctx, X, S, V, d_cols, K, d_sa));
    BA_TRY(launch_col_percentiles(ctx, d_sa, K, S, d_pct, 2, d_qa));
    hipLaunchKernelGGL(k_conv_hdi, dim3((unsigned)K), dim3(CV_TB), 0, st, d_sa, S, inc, d_hdi);
    BA_HIP(hipGetLastError());
    if (diag) {
        double *d_w, *d_sb, *d_rm;
        int64_t *d_off;
        BA_TRY(ctx->scratch(SL_CV_W, (size_t)K * CV_NT * n2, &d_w));
        BA_TRY(ctx->scratch(SL_CV_SB, (size_t)K * n2, &d_sb));
        BA_TRY(ctx->scratch(SL_CV_RM, (size_t)K * CV_NT * M * 4, &d_rm));
        BA_TRY(ctx->scratch(SL_CV_OFF, (size_t)K, &d_off));
        const dim3 eg(cv_blocks(n2), (unsigned)K);
        hipLaunchKernelGGL(k_conv_write_raw, eg, dim3(CV_TB), 0, st, X, C, D, V, d_cols, h, d_w);
        hipLaunchKernelGGL(k_conv_iota, dim3(cv_blocks(K)), dim3(CV_TB), 0, st, d_off, K, (int64_t)0, CV_NT * n2);
        BA_TRY(launch_col_sort(ctx, d_w, n2, 1, d_off, K, d_sb));
        BA_TRY(launch_col_percentiles(ctx, d_sb, K, n2, d_pct + 2, 1, d_med));
        hipLaunchKernelGGL(k_conv_write_derived, eg, dim3(CV_TB), 0, st, d_w, n2, d_cm, d_qa, d_med);
        hipLaunchKernelGGL(k_conv_iota, dim3(cv_blocks(K)), dim3(CV_TB), 0, st, d_off, K, 5 * n2, CV_NT * n2);
        BA_TRY(launch_col_sort(ctx, d_w, n2, 1, d_off, K, d_sa));   // (the sorted column is no longer needed)
        hipLaunchKernelGGL(k_conv_rank_z, eg, dim3(CV_TB), 0, st, d_w, CV_NT * n2, d_sb, n2, d_w + 4 * n2, CV_NT * n2,
                           (double *)nullptr);
        hipLaunchKernelGGL(k_conv_rank_z, eg, dim3(CV_TB), 0, st, d_w + 5 * n2, CV_NT * n2, d_sa, n2, d_w + 5 * n2, CV_NT * n2,
                           (double *)nullptr);
        BA_CHECK(K * CV_NT * M < (int64_t)0x7fffffff, BEATAMD_EINVAL, "convergence_summary: batch too large");
        hipLaunchKernelGGL(k_conv_moments, dim3((unsigned)(K * CV_NT * M)), dim3(CV_TB), 0, st, d_w, (const int64_t *)nullptr, h,
                           (int64_t)1, d_rm);
        hipLaunchKernelGGL(k_conv_rhat, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, st, K, M, h, d_rm, d_rhat);
        BA_HIP(hipGetLastError());
        // Geyer's sequence on lags computed on demand: [0, B), then four times as many, for the groups still scanning
        std::vector<int32_t> act, state;
        for (int64_t k = 0; k < K; k++)
            for (int t = 0; t < 5; t++) act.push_back((int32_t)(k * CV_NT + t));
        if (!(tau_floor > 0.0)) tau_floor = 1.0 / std::log10((double)(M * h));
        int64_t have = 0, ld = 0, nround = 0;
        int cur = 0;
        double *d_mac = nullptr;
        while (!act.empty()) {
            const int64_t A = (int64_t)act.size();
            const int64_t want = std::min<int64_t>(h, have == 0 ? std::max<int64_t>(first_lags, 2) : have * 4);
            int32_t *d_act, *d_state;
            double *d_new, *d_ac, *d_rho;
            BA_TRY(ctx->scratch(SL_CV_ACT, (size_t)A * 2, &d_act));
            BA_TRY(ctx->scratch(SL_CV_STATE, (size_t)A, &d_state));
            BA_TRY(ctx->scratch(cur ? SL_CV_MAC1 : SL_CV_MAC0, (size_t)A * want, &d_new));
            BA_TRY(ctx->scratch(SL_CV_AC, (size_t)A * M * (want - have), &d_ac));
            BA_TRY(ctx->scratch(SL_CV_RHO, (size_t)A * want, &d_rho));
            // act[a] and, behind them, the rows of the previous round's table they had (state holds those from last round)
            std::vector<int32_t> up(act);
            up.insert(up.end(), state.begin(), state.end());
            up.resize((size_t)A * 2, 0);
            BA_HIP(hipMemcpyAsync(d_act, up.data(), up.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
            BA_HIP(hipStreamSynchronize(st));
            if (have)
                hipLaunchKernelGGL(k_conv_regroup, dim3(cv_blocks(have), (unsigned)A), dim3(CV_TB), 0, st, d_mac, ld, d_act + A, have,
                                   d_new, want);
            BA_TRY(cv_lags(ctx, d_w, d_rm, d_act, A * M, M, h, have, want - have, d_ac));
            hipLaunchKernelGGL(k_conv_lagmean, dim3(cv_blocks(want - have), (unsigned)A), dim3(CV_TB), 0, st, d_ac, M, want - have,
                               d_new, want, have);
            hipLaunchKernelGGL(k_conv_geyer, dim3((unsigned)((A + 63) / 64)), dim3(64), 0, st, A, d_act, M, h, d_rm, d_new, d_rho,
                               want, want, tau_floor, d_ess, d_state);
            BA_HIP(hipGetLastError());
            std::vector<int32_t> fl;
            BA_TRY(cv_readback(ctx, d_state, (size_t)A, fl));
            std::vector<int32_t> next;
            state.clear();
            for (int64_t a = 0; a < A; a++)
                if (fl[a]) {
                    next.push_back(act[a]);
                    state.push_back((int32_t)a);
                }
            BA_CHECK(next.empty() || want < h, BEATAMD_EINVAL, "convergence_summary: internal: a scan wants more than all lags");
            act.swap(next);
            d_mac = d_new;
            ld = have = want;
            cur ^= 1;
            nround++;
        }
        if (rounds) *rounds = std::max(*rounds, nround);
    }
    hipLaunchKernelGGL(k_conv_finish, dim3(cv_blocks(K)), dim3(CV_TB), 0, st, K, S, d_cm, d_hdi, d_ess, d_rhat, flags, (int)diag, out);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int64_t convergence_batch(int64_t C, int64_t D, int64_t K)
{
    // doubles a variable needs: six row sets, two sorted copies, the lag tables (at most another row set and a half)
    const int64_t S = C * D, per = 10 * std::max<int64_t>(S, 1) * (int64_t)sizeof(double);
    const int64_t by_budget = std::max<int64_t>(1, CV_WORKSPACE_BYTES / per);
    const int64_t by_grid = std::max<int64_t>(1, (int64_t)0x7ffffff0 / (CV_NT * 2 * std::max<int64_t>(C, 1)));
    return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(K, 16384), std::min(by_budget, by_grid)));
}

int launch_convergence_summary(beatamd_ctx *ctx, int64_t C, int64_t D, int64_t V, const double *X, int64_t K,
                               const int64_t *d_cols, double hdi_prob, double tau_floor, int64_t var_batch, int64_t first_lags,
                               double *out, int32_t *flags, int64_t *rounds)
{
    if (K == 0) return BEATAMD_OK;
    const int64_t S = C * D;
    BA_CHECK(S <= MG_SORT_MAX_N, BEATAMD_EINVAL, "convergence_summary: %lld samples a variable, at most %lld", (long long)S,
             (long long)MG_SORT_MAX_N);
    ScopedTimer tm(ctx, "convergence_summary");
    const int64_t inc = std::min<int64_t>((int64_t)std::floor(hdi_prob * (double)S), S - 1);
    const int64_t batch = var_batch > 0 ? std::min<int64_t>(var_batch, 16384) : convergence_batch(C, D, K);
    if (rounds) *rounds = 0;
    for (int64_t k0 = 0; k0 < K; k0 += batch) {
        const int64_t kb = std::min(batch, K - k0);
        BA_TRY(cv_summary_batch(ctx, C, D, V, X, kb, d_cols + k0, inc, tau_floor, first_lags, out + k0 * CV_NCOL, flags + k0, rounds));
    }
    return BEATAMD_OK;
}

}  // namespace beatamd
