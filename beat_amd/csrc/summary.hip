// summary.hip -- posterior diagnostics of a whole stage population: variance reductions from the cached misfits,
// standardized residuals, and running moments of an ensemble of synthetics.  The forward model and the quadratic
// forms are the likelihood's own kernels (capi.cpp); what is here is the arithmetic the reference does after them.
#include "kernels.hpp"
#include "raster.hpp"

namespace beatamd {

// seismic.py:610-620 / geodetic.py:494-505: VR = 1 - nom / denom, plain IEEE (a zero denominator gives what the
// division gives; the NaN row of a flagged chain stays NaN)
__global__ void __launch_bounds__(256) k_variance_reduction(int64_t C, int64_t n, const double *nom, int64_t ld,
                                                           const double *denom, double *VR)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C * n) return;
    const int64_t c = i / n, k = i - c * n;
    VR[i] = 1.0 - nom[c * ld + k] / denom[k];
}

int launch_variance_reduction(beatamd_ctx *ctx, int64_t C, int64_t n, const double *nom, int64_t ld, const double *denom,
                              double *VR)
{
    if (C * n == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_variance_reduction, dim3((unsigned)((C * n + 255) / 256)), dim3(256), 0, ctx->stream, C, n, nom, ld,
                       denom, VR);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// seismic.py:560-561 / geodetic.py:539-541: inv(chol(exp(2h) C)) . r = exp(-h) (inv(chol(C)) . r).  The scalar operator
// and the scale: out[c,t,k] = exp(-hp[c,t]) * (S[t] * X[c,t,k]); S == nullptr: X holds the dense product already (it may
// be `out` itself), hp == nullptr: no scale
__global__ void __launch_bounds__(256) k_standardize(int64_t total, int64_t T, int64_t N, const double *S, const double *hp,
                                                    const double *X, double *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t ct = i / N;
    double z = X[i];
    if (S) z = S[ct % T] * z;
    if (hp) z = exp(-hp[ct]) * z;
    out[i] = z;
}

int launch_standardize(beatamd_ctx *ctx, int64_t C, int64_t T, int64_t N, const double *S, const double *hp, const double *X,
                       double *out)
{
    const int64_t total = C * T * N;
    if (total == 0) return BEATAMD_OK;
    BA_CHECK((total + 255) / 256 < (int64_t)0x7fffffff, BEATAMD_EINVAL, "standardize: too many elements");
    hipLaunchKernelGGL(k_standardize, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, total, T, N, S, hp, X,
                       out);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// Running moments of the columns of X [C, M] (plotting/seismic.py:395-451 collects the synthetics of an ensemble; its
// callers take mean and envelope): state [5, M] = (mean, M2, min, max, spare).  Lane <-> two neighbouring columns, the
// rows taken in row order with exactly
//     d = x - m;  m = m + d / n;  M2 = M2 + d * (x - m)           (Welford; n = rows seen including this one)
// so the state after a call does not depend on how the rows were cut into calls.  MR rows' loads are in flight per lane
// before the first is used; no LDS, no atomics: a stream of C * M * 8 bytes.  VEC: M is even and X 16-byte aligned, a
// lane's two columns are one 16-byte load; otherwise two 8-byte loads, the second guarded at an odd M's last column.
constexpr int MOM_ROWS = 8;

template <bool VEC>
__global__ void __launch_bounds__(64) k_ensemble_moments(int64_t C, int64_t M, const double *X, double *state, int64_t n_seen)
{
#pragma clang fp contract(off)
    const int64_t j = ((int64_t)blockIdx.x * 64 + threadIdx.x) * 2;
    if (j >= M) return;
    const bool two = j + 1 < M;
    double m0 = 0.0, s0 = 0.0, lo0 = __builtin_inf(), hi0 = -__builtin_inf();
    double m1 = 0.0, s1 = 0.0, lo1 = __builtin_inf(), hi1 = -__builtin_inf();
    if (n_seen > 0) {
        m0 = state[j]; s0 = state[M + j]; lo0 = state[2 * M + j]; hi0 = state[3 * M + j];
        if (two) { m1 = state[j + 1]; s1 = state[M + j + 1]; lo1 = state[2 * M + j + 1]; hi1 = state[3 * M + j + 1]; }
    }
    const double *x = X + j;
    for (int64_t r0 = 0; r0 < C; r0 += MOM_ROWS) {
        double a[MOM_ROWS], b[MOM_ROWS];
#pragma unroll
        for (int u = 0; u < MOM_ROWS; u++) {
            const int64_t r = r0 + u < C ? r0 + u : C - 1;      // (behind the last row: that row again, not used)
            if (VEC) {
                const double2 v = *reinterpret_cast<const double2 *>(x + r * M);
                a[u] = v.x; b[u] = v.y;
            } else {
                a[u] = x[r * M];
                b[u] = two ? x[r * M + 1] : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < MOM_ROWS; u++) {
            if (r0 + u < C) {
                const double n = (double)(n_seen + r0 + u + 1);
                const double d0 = a[u] - m0;
                m0 = m0 + d0 / n;
                s0 = s0 + d0 * (a[u] - m0);
                lo0 = a[u] < lo0 ? a[u] : lo0;
                hi0 = a[u] > hi0 ? a[u] : hi0;
                const double d1 = b[u] - m1;
                m1 = m1 + d1 / n;
                s1 = s1 + d1 * (b[u] - m1);
                lo1 = b[u] < lo1 ? b[u] : lo1;
                hi1 = b[u] > hi1 ? b[u] : hi1;
            }
        }
    }
    const double seen = (double)(n_seen + C);   // the spare row: rows seen so far
    state[j] = m0; state[M + j] = s0; state[2 * M + j] = lo0; state[3 * M + j] = hi0; state[4 * M + j] = seen;
    if (two) {
        state[j + 1] = m1; state[M + j + 1] = s1; state[2 * M + j + 1] = lo1; state[3 * M + j + 1] = hi1;
        state[4 * M + j + 1] = seen;
    }
}

int launch_ensemble_moments(beatamd_ctx *ctx, int64_t C, int64_t M, const double *X, double *state, int64_t n_seen)
{
    if (C == 0 || M == 0) return BEATAMD_OK;
    const int64_t nblocks = ((M + 1) / 2 + 63) / 64;
    BA_CHECK(nblocks < (int64_t)0x7fffffff, BEATAMD_EINVAL, "ensemble_moments: too many columns");
    ScopedTimer tm(ctx, "moments");
    if (M % 2 == 0 && (uintptr_t)X % 16 == 0)
        hipLaunchKernelGGL(k_ensemble_moments<true>, dim3((unsigned)nblocks), dim3(64), 0, ctx->stream, C, M, X, state, n_seen);
    else
        hipLaunchKernelGGL(k_ensemble_moments<false>, dim3((unsigned)nblocks), dim3(64), 0, ctx->stream, C, M, X, state, n_seen);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// mean, std = sqrt(M2 / n) (numpy.std, ddof = 0), min, max from the state
__global__ void __launch_bounds__(256) k_moments_finish(int64_t M, const double *state, double n, double *mean, double *std,
                                                       double *mn, double *mx)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    mean[j] = state[j];
    std[j] = sqrt(state[M + j] / n);
    mn[j] = state[2 * M + j];
    mx[j] = state[3 * M + j];
}

int launch_moments_finish(beatamd_ctx *ctx, int64_t M, const double *state, int64_t n, double *mean, double *std, double *mn,
                          double *mx)
{
    if (M == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_moments_finish, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, ctx->stream, M, state, (double)n, mean,
                       std, mn, mx);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ---- density grid of an ensemble of traces (plotting/seismic.py:255-316 fuzzy_waveforms; plotting/common.py:619-801
// draw_line_on_array / _weighted_line; utility.py:1556 positions2idxs).  Every trace Y[e, t, :] is drawn as N - 1
// anti-aliased segments into an image of its own -- a pixel keeps the value of the highest-numbered segment that writes
// it -- and the image is added to grid[t]; traces in ensemble order.  The rasteriser is raster.hpp's, the reference's
// arithmetic operation by operation: the grid is the reference's bit for bit.  What is here is where a workgroup's
// segments come from: the time axis is uniform.
struct TdArgs {
    int64_t E, T, N;
    const double *Y, *tmin, *extent;   // [E,T,N], [T], [T,4] = (xmin, xmax, ymin, ymax)
    const int64_t *ranges;             // [E,T,2] = (first sample, count) of every trace, or nullptr: all N samples
    double deltat, linewidth;
    int ny, nx, strip, pad;
    double *grid;                      // [T,ny,nx]
    int *status;
};

// the samples [*lo, *hi) of trace `tr` = e * T + t that its range (first, count) leaves inside [0, N); false: fewer than
// two, the trace draws nothing
__device__ __forceinline__ bool td_range(const TdArgs &a, int64_t tr, int64_t *lo, int64_t *hi)
{
    const int64_t f = a.ranges[2 * tr], n = a.ranges[2 * tr + 1];
    if (n < 2 || f >= a.N || f < -((int64_t)1 << 62) || (f < 0 && n <= -f)) return false;   // (no sum that can overflow)
    *lo = f > 0 ? f : 0;
    *hi = n >= a.N - f ? a.N : f + n;
    return true;
}

// every sample's row index and every time's column index (rs_index_status).  k_trace_density does not start on a raised word.
// With ranges only the samples inside their trace's range are looked at, each with its time (a time outside every range
// is never drawn)
template <bool RANGED>
__device__ __forceinline__ void td_check(const TdArgs &a)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.E * a.T * a.N) return;
    const int64_t j = i % a.N, t = (i / a.N) % a.T;
    const double *ext = a.extent + 4 * t;
    if (RANGED) {
        int64_t lo, hi;
        if (!td_range(a, i / a.N, &lo, &hi) || j < lo || j >= hi) return;
    }
    const double ystep = (ext[3] - ext[2]) / (double)(a.ny - 1);
    int bad = rs_index_status(rs_cell(a.Y[i], ext[2], ystep), a.ny - 1);
    if (RANGED || i < a.T * a.N) {           // the time axis is the same for every trace of a target
        const double xstep = (ext[1] - ext[0]) / (double)(a.nx - 1);
        const double c = rs_cell(a.tmin[t] + (double)j * a.deltat, ext[0], xstep);
        bad |= xstep > 0.0 ? rs_index_status(c, a.nx - 1) : ST_LINE_NONFINITE;
    }
    if (bad) atomicOr(a.status, bad);
}

__global__ void __launch_bounds__(256) k_trace_density_check(TdArgs a) { td_check<false>(a); }
__global__ void __launch_bounds__(256) k_trace_density_check_ranged(TdArgs a) { td_check<true>(a); }

// The set-up (raster.hpp) of the RS_THREADS segments of trace y from seg0 on (the last is ihi) for the workgroup's columns
// [s0, s1) and all rows; segment i joins samples i - 1 and i.  -> its pairs
__device__ __forceinline__ int td_setup(const TdArgs &a, RsSetup &S, const double *y, int64_t seg0, int64_t ihi, double tmin,
                                        double xmin, double xstep, double ymin, double ystep, int s0, int s1)
{
#pragma clang fp contract(off)
    const int64_t i = seg0 + threadIdx.x;
    const bool have = i <= ihi;
    int c0 = 0, r0 = 0, c1 = 0, r1 = 0;
    if (have) {
        c0 = (int)rs_cell(tmin + (double)(i - 1) * a.deltat, xmin, xstep);
        c1 = (int)rs_cell(tmin + (double)i * a.deltat, xmin, xstep);
        r0 = (int)rs_cell(y[i - 1], ymin, ystep);
        r1 = (int)rs_cell(y[i], ymin, ystep);
    }
    return rs_setup(S, have, c0, r0, c1, r1, a.linewidth, s0, s1, 0, a.ny - 1);
}

// One workgroup <-> (a strip of grid columns, a target); it walks the traces in ensemble order, so every pixel's sum has
// the reference's order without atomics on doubles, and the strip of grid[t] is the workgroup's alone.  The time axis is
// uniform: the segments that can touch the strip (widened by `pad` columns, the reach of the widest line) are one index
// range, found by bisection once.  Per trace: pass 0 over the range in chunks of RS_THREADS segments, then pass 1 (with
// one chunk, on the set-up that pass 0 left).  The result does not depend on the strip width or on the chunking.
// RANGED: the kernel with per-trace ranges (k_trace_density_ranged); without them the code is the plain kernel's
template <bool RANGED>
__device__ __forceinline__ void td_draw(const TdArgs &a, uint32_t *td_owner, RsSetup &S)
{
#pragma clang fp contract(off)
    if (*(volatile int *)a.status & (ST_LINE_OOB | ST_LINE_NONFINITE)) return;   // (k_trace_density_check, uniform)
    const int t = blockIdx.y, tid = threadIdx.x;
    const int s0 = blockIdx.x * a.strip, s1 = min(s0 + a.strip, a.nx - 1);
    if (s0 >= s1) return;
    const double *ext = a.extent + 4 * t;
    const double xmin = ext[0], ymin = ext[2], tmin = a.tmin[t];
    const double xstep = (ext[1] - xmin) / (double)(a.nx - 1), ystep = (ext[3] - ymin) / (double)(a.ny - 1);
    for (int k = tid; k < a.ny * a.strip; k += RS_THREADS) td_owner[k] = 0u;
    // first sample whose column is >= lo / > hi (columns do not decrease with the sample index)
    const double clo = (double)(s0 - a.pad), chi = (double)(s1 - 1 + a.pad);
    int64_t jlo = 0, n = a.N;
    while (n > 0) {
        const int64_t h = n / 2;
        if (rs_cell(tmin + (double)(jlo + h) * a.deltat, xmin, xstep) < clo) { jlo += h + 1; n -= h + 1; } else n = h;
    }
    int64_t jhi = jlo;
    n = a.N - jlo;
    while (n > 0) {
        const int64_t h = n / 2;
        if (rs_cell(tmin + (double)(jhi + h) * a.deltat, xmin, xstep) <= chi) { jhi += h + 1; n -= h + 1; } else n = h;
    }
    const int64_t ilo = jlo > 1 ? jlo : 1, ihi = jhi < a.N - 1 ? jhi : a.N - 1;    // segment i joins samples i - 1 and i
    if (ilo > ihi) return;
    const bool one = ihi - ilo < RS_THREADS;
    double *g = a.grid + (int64_t)t * a.ny * a.nx;
    __syncthreads();
    for (int64_t e = 0; e < a.E; e++) {
        const double *y = a.Y + (e * a.T + t) * a.N;
        int total = 0;
        // RANGED: the trace's own range (first sample, count) cut to [0, N) -- its segments are first + 1 ... first + count - 1,
        // those of them that can touch the strip lo ... hi (uniform over the workgroup: the barriers stay matched)
        int64_t lo = ilo, hi = ihi;
        bool single = one;
        if (RANGED) {
            int64_t rf, rend;
            if (!td_range(a, e * a.T + t, &rf, &rend)) continue;
            lo = ilo > rf + 1 ? ilo : rf + 1;
            hi = ihi < rend - 1 ? ihi : rend - 1;
            if (lo > hi) continue;
            single = hi - lo < RS_THREADS;
        }
        for (int64_t seg0 = lo; seg0 <= hi; seg0 += RS_THREADS) {
            total = td_setup(a, S, y, seg0, hi, tmin, xmin, xstep, ymin, ystep, s0, s1);
            rs_pass<0>(S, td_owner, a.strip, g, nullptr, a.nx, seg0, total, s0, s1, 0, a.ny - 1);
            __syncthreads();
        }
        for (int64_t seg0 = lo; seg0 <= hi; seg0 += RS_THREADS) {
            if (!single) total = td_setup(a, S, y, seg0, hi, tmin, xmin, xstep, ymin, ystep, s0, s1);
            rs_pass<1>(S, td_owner, a.strip, g, nullptr, a.nx, seg0, total, s0, s1, 0, a.ny - 1);
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(RS_THREADS) k_trace_density(TdArgs a)
{
    extern __shared__ uint32_t td_owner[];
    __shared__ RsSetup S;
    td_draw<false>(a, td_owner, S);
}

__global__ void __launch_bounds__(RS_THREADS) k_trace_density_ranged(TdArgs a)
{
    extern __shared__ uint32_t td_owner[];
    __shared__ RsSetup S;
    td_draw<true>(a, td_owner, S);
}

// the owner map's share of the 160 KiB of LDS (RsSetup takes 10 KiB)
constexpr int TD_LDS_BYTES = 150 * 1024, TD_STRIP = 32, TD_STRIP_MIN = 8;

int launch_trace_density(beatamd_ctx *ctx, int64_t E, int64_t T, int64_t N, const double *Y, const double *tmin, double deltat,
                         const double *extent, int64_t ny, int64_t nx, double linewidth, double *grid)
{
    return launch_trace_density(ctx, E, T, N, Y, tmin, deltat, extent, ny, nx, linewidth, grid, nullptr);
}

int launch_trace_density(beatamd_ctx *ctx, int64_t E, int64_t T, int64_t N, const double *Y, const double *tmin, double deltat,
                         const double *extent, int64_t ny, int64_t nx, double linewidth, double *grid, const int64_t *ranges)
{
    BA_TRY(rs_check_args("trace_density", ny, nx, linewidth));
    BA_CHECK(N >= 2 && N < (int64_t)0x7fffffff, BEATAMD_EINVAL, "trace_density: %lld samples (at least 2)", (long long)N);
    BA_CHECK(deltat > 0.0 && deltat <= DBL_MAX, BEATAMD_EINVAL, "trace_density: deltat %g", deltat);
    BA_CHECK(E >= 0 && T >= 0 && T <= 65535, BEATAMD_EINVAL, "trace_density: bad ensemble or target count");
    if (E == 0 || T == 0) return BEATAMD_OK;
    const int64_t nchk = (E * T * N + 255) / 256;
    BA_CHECK(nchk < (int64_t)0x7fffffff, BEATAMD_EINVAL, "trace_density: too many samples in one call");
    TdArgs a;
    a.E = E; a.T = T; a.N = N; a.Y = Y; a.ranges = ranges; a.tmin = tmin; a.extent = extent; a.deltat = deltat; a.linewidth = linewidth;
    a.ny = (int)ny; a.nx = (int)nx; a.grid = grid; a.status = ctx->d_status;
    a.pad = rs_pad(linewidth);
    // strip: TD_STRIP columns where segments are long (a workgroup per trace has a fixed cost: fewer workgroups), narrower
    // where samples are dense, so that the (strip + 2 pad) N / nx segments of a strip fill 3/4 of one chunk -- a second
    // chunk costs a second set-up in both passes (measured, 500 x 500, width 7, 200 x 64 traces: N = 4096 16.1 ms at 32
    // columns, 18.1 at 24, 11.4 at 12; N = 120 3.1 ms at 32, 4.0 at 12) -- and as the owner map allows.
    // BEATAMD_TD_STRIP: a test knob, the result does not change
    const int fit = (int)(TD_LDS_BYTES / (4 * ny));
    const int64_t dense = (int64_t)(RS_THREADS * 3 / 4) * nx / N - 2 * a.pad;
    const int want = GfKnobs::get(gf_knobs(ctx).td_strip, (int)std::max<int64_t>(TD_STRIP_MIN, std::min<int64_t>(TD_STRIP, dense)));
    a.strip = std::max(1, std::min(std::min(want, fit), (int)nx));
    const size_t lds = (size_t)ny * a.strip * sizeof(uint32_t);
    const auto check = ranges ? k_trace_density_check_ranged : k_trace_density_check;
    const auto draw = ranges ? k_trace_density_ranged : k_trace_density;
    if (lds + sizeof(RsSetup) > 64 * 1024)
        BA_HIP(hipFuncSetAttribute((const void *)draw, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ScopedTimer tm(ctx, "density");
    hipLaunchKernelGGL(check, dim3((unsigned)nchk), dim3(256), 0, ctx->stream, a);
    BA_HIP(hipGetLastError());
    hipLaunchKernelGGL(draw, dim3((unsigned)((nx - 1 + a.strip - 1) / a.strip), (unsigned)T), dim3(RS_THREADS), lds, ctx->stream, a);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
