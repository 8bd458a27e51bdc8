// seislib.hip -- the producer of the seismic FFI Green's-function library (T, P, D, S, N) that the stacking kernels stream:
// what the reference builds with one process per patch and a Python loop over targets x durations x starttimes
// (beat/ffi/base.py:1005-1254 seis_construct_gf_linear / _process_patch_seismic, through heart.taper_filter_traces and
// post_process_trace, beat/heart.py:3466-3525, 4242-4323).  The elementary waveforms (pyrocko's engine.process on a GF
// store) come from the caller; everything after them is done here, in HBM.
//
// THE ARITHMETIC CONTRACT (tests/seislib_ref.py restates it in numpy, operation by operation).  FP64, contraction off,
// no atomics, every index checked before it is used.
//
// Inputs   responses [T, P, L]: the unit-slip response of every (target, patch) for an impulsive source-time function,
//          sampled at deltat; tmins [T, P]: the time of sample 0, relative to the event's origin time, which lies on the
//          sample grid (the reference's patch.time = event.time, base.py:1010); arrival_times [T]: the event's phase
//          arrival per target (the library's _tmins, base.py:1044); durations [D], starttimes [S]; a taper (a, b, c, d);
//          up to SL_MAX_STAGES filter stages.
//
// Source-time function, per duration dur: the half-sinusoid of k_moment_rate (momentrate.hip) with t0 = 0, t1 = dur,
//          anchor -1 as base.py:1013 sets it:  k1 = rint(dur / deltat), nt = k1 + 1;  nt == 1: a = [1];  otherwise
//          a_i = mr_amplitude(i) (stf.hpp, the same device function) divided by S, S in the same fixed order (lane l adds
//          a_l, a_{l+64}, ... from 0.0, the 64 lane sums folded 32 / 16 / ... / 1).  The amplitudes depend on the duration
//          alone: one table A [D, ntmax] (k_stf_table), zero beyond nt.  pyrocko's discretize_t AS RECALLED, UNVERIFIED.
//
// Convolution   yc[n] = sum_{i = 0}^{nt - 1} a_i g[n - i], i ascending from 0.0, n in [0, Lc), Lc = L + nt - 1 (terms
//          with n - i outside [0, L) are left out; they would add zeros).
//
// Filter cascade over exactly the Lc samples, stage after stage.  A stage is (b[0..m], a[0..m], demean), a[0] = 1,
//          3 <= m + 1 <= SL_MAX_TAPS.  demean subtracts (sum of the stage's input, n ascending from 0.0) / Lc (DEVIATION:
//          numpy's mean is a pairwise sum).  The recurrence is direct form II transposed with zero initial state:
//              y    = z[0] + b[0] x
//              z[k] = (z[k+1] + x b[k+1]) - y a[k+1],  k = 0 .. m - 2
//              z[m-1] = x b[m] - y a[m]
//          which is scipy.signal.lfilter's order (tests/test_seislib_host.py holds the bit-for-bit check).
//
// Window, per (t, p, s): the host hands over i0 [T, P, S] = floor((arrival_times[t] - starttimes[s] + b - tmins[t, p]) /
//          deltat) (chop's snap = (floor, floor), heart.py:3522) and w0 [T, P, S], the cosine fade-in at the time of sample
//          i0 where that lies below the shifted taper edge b', 1 otherwise (only sample 0 of a [b, c] cut can lie in the
//          fade).  lib[t, p, d, s, n] = yf[d][i0 + n] if 0 <= i0 + n < Lc, else 0 (the reference's
//          extend(fillmethod="zeros") after filtering); sample 0 is multiplied by w0.  pyrocko's extend / taper / chop AS
//          RECALLED, UNVERIFIED.
//
// The result does not depend on the launch shape or on patch_block: one lane owns a trace from its first sample to its
// last, and every sum above has one order.
#include "kernels.hpp"
#include "stf.hpp"
#include "wave.hpp"

namespace beatamd {

// ---- k_stf_table: one wavefront <-> one duration.  nt [D], A [D, ntmax] (zero beyond nt).  A duration whose nt does not
// fit ntmax gets nt = 0 and a zero row (the entry point refuses it ahead of the launch).
__global__ void __launch_bounds__(64) k_stf_table(int64_t D, const double *durations, double deltat, int64_t ntmax, int32_t *nt_out,
                                                  double *A)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const int64_t d = blockIdx.x;
    if (d >= D) return;
    const double dur = durations[d], r1 = rint(dur / deltat);
    double *row = A + d * ntmax;
    const bool fits = r1 >= 0.0 && r1 + 1.0 <= (double)ntmax;
    const int64_t nt = fits ? (int64_t)r1 + 1 : 0;
    if (lane == 0) nt_out[d] = (int32_t)nt;
    for (int64_t i = nt + lane; i < ntmax; i += 64) row[i] = 0.0;
    if (nt == 0) return;
    if (nt == 1) {
        if (lane == 0) row[0] = 1.0;
        return;
    }
    const double t0 = 0.0, t1 = dur, tmin = 0.0, w = 3.14159265358979323846 / dur;
    double part = 0.0;
    for (int64_t i = lane; i < nt; i += 64) part = part + mr_amplitude(i, tmin, t0, t1, w, deltat);
    part = wave_butterfly<OpAdd>(part);
    for (int64_t i = lane; i < nt; i += 64) row[i] = mr_amplitude(i, tmin, t0, t1, w, deltat) / part;
}

int launch_stf_table(beatamd_ctx *ctx, int64_t D, const double *durations, double deltat, int64_t ntmax, int32_t *nt, double *A)
{
    if (D == 0) return BEATAMD_OK;
    BA_CHECK(D < (int64_t)0x7fffffff && ntmax >= 1 && ntmax <= SL_NT_MAX, BEATAMD_EINVAL, "stf_table: bad size");
    ScopedTimer tm(ctx, "stf_table");
    hipLaunchKernelGGL(k_stf_table, dim3((unsigned)D), dim3(64), 0, ctx->stream, D, durations, deltat, ntmax, nt, A);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// the traces of a block of patches [p0, p0 + pb) are numbered q = (t pb + pl) D + d; row q of Y has Lcmax samples, of which
// the first Lc = L + nt[d] - 1 are the trace and the rest stay zero
struct SlTrace {
    int64_t t, pl, d, len;
};
__device__ __forceinline__ SlTrace sl_trace(int64_t q, int64_t pb, int64_t D, int64_t L, const int32_t *nt, int64_t ntmax,
                                            int64_t Lcmax)
{
    SlTrace r;
    r.d = q % D;
    const int64_t tp = q / D;
    r.pl = tp % pb;
    r.t = tp / pb;
    int64_t n = nt[r.d];
    n = n < 1 ? 1 : (n > ntmax ? ntmax : n);
    r.len = L + n - 1;
    if (r.len > Lcmax) r.len = Lcmax;
    return r;
}

// ---- k_stf_convolve: one workgroup <-> one trace q, lanes along the samples (coalesced reads of g, coalesced writes)
__global__ void __launch_bounds__(256) k_stf_convolve(int64_t Q, int64_t P, int64_t p0, int64_t pb, int64_t L, const double *X,
                                                      int64_t D, int64_t ntmax, const int32_t *nt, const double *A, int64_t Lcmax,
                                                      double *Y)
{
#pragma clang fp contract(off)
    const int64_t q = blockIdx.x;
    if (q >= Q) return;
    const SlTrace tr = sl_trace(q, pb, D, L, nt, ntmax, Lcmax);
    const double *g = X + (tr.t * P + p0 + tr.pl) * L, *a = A + tr.d * ntmax;
    const int64_t n_t = tr.len - L + 1;
    double *y = Y + q * Lcmax;
    for (int64_t n = threadIdx.x; n < Lcmax; n += 256) {
        double s = 0.0;
        if (n < tr.len) {
            const int64_t ilo = n - (L - 1) > 0 ? n - (L - 1) : 0, ihi = n < n_t - 1 ? n : n_t - 1;
            for (int64_t i = ilo; i <= ihi; i++) s = s + a[i] * g[n - i];
        }
        y[n] = s;
    }
}

int launch_stf_convolve(beatamd_ctx *ctx, int64_t T, int64_t P, int64_t p0, int64_t pb, int64_t L, const double *X, int64_t D,
                        int64_t ntmax, const int32_t *nt, const double *A, int64_t Lcmax, double *Y)
{
    const int64_t Q = T * pb * D;
    if (Q == 0) return BEATAMD_OK;
    BA_CHECK(Q < (int64_t)0x7fffffff && p0 >= 0 && pb >= 1 && p0 + pb <= P && L >= 1 && Lcmax >= L && Lcmax <= L + ntmax - 1,
             BEATAMD_EINVAL, "stf_convolve: bad block of patches or trace length");
    ScopedTimer tm(ctx, "stf_convolve");
    hipLaunchKernelGGL(k_stf_convolve, dim3((unsigned)Q), dim3(256), 0, ctx->stream, Q, P, p0, pb, L, X, D, ntmax, nt, A, Lcmax, Y);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ---- k_trace_filter: one stage of the cascade, in place.  One lane <-> one trace, 64 traces a workgroup.  Tiles of 64
// traces x 64 samples go through LDS so that the global loads and stores run along the sample axis; a tile row is padded by
// one double, so the lanes' column reads (ds_read_b64, 32 lanes a group) hit 64 distinct banks.  The recurrence state is
// NTAPS - 1 registers: the tap loops unroll over the compile-time tap count, nothing is indexed at run time.
constexpr int SL_TILE = 64, SL_TILE_LD = SL_TILE + 1;

// rows [q0, q0 + nrows) x columns [c0, c0 + 64) of Y into the tile, zeros outside.  Every load is unconditional at an
// address clamped into the block (a branch around a load would make the wavefront wait for each row in turn): sixteen rows
// are in flight before their LDS stores.
__device__ __forceinline__ void sl_tile_load(double *tile, const double *Y, int64_t q0, int nrows, int64_t c0, int64_t Lcmax,
                                             int lane)
{
    const bool col_ok = c0 + lane < Lcmax;
    const int64_t col = col_ok ? c0 + lane : Lcmax - 1;
    for (int j0 = 0; j0 < SL_TILE; j0 += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = Y[(q0 + (j0 + u < nrows ? j0 + u : nrows - 1)) * Lcmax + col];
#pragma unroll
        for (int u = 0; u < 16; u++) tile[(j0 + u) * SL_TILE_LD + lane] = (j0 + u < nrows && col_ok) ? v[u] : 0.0;
    }
}

template <int NTAPS>
__global__ void __launch_bounds__(64) k_trace_filter(int64_t Q, int64_t D, int64_t L, int64_t ntmax, const int32_t *nt,
                                                     int64_t Lcmax, SlStage st, double *Y)
{
#pragma clang fp contract(off)
    __shared__ double tile[SL_TILE * SL_TILE_LD];
    const int lane = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * SL_TILE, q = q0 + lane;
    if (q0 >= Q) return;
    const int nrows = (int)(Q - q0 < SL_TILE ? Q - q0 : SL_TILE);
    const int64_t len = q < Q ? sl_trace(q, 1, D, L, nt, ntmax, Lcmax).len : 0;
    double *mine = tile + lane * SL_TILE_LD;
    double mean = 0.0;
    if (st.demean) {
        double sum = 0.0;
        for (int64_t c0 = 0; c0 < Lcmax; c0 += SL_TILE) {
            sl_tile_load(tile, Y, q0, nrows, c0, Lcmax, lane);
            __syncthreads();
            for (int k = 0; k < SL_TILE; k++)
                if (c0 + k < len) sum = sum + mine[k];
            __syncthreads();
        }
        if (len > 0) mean = sum / (double)len;
    }
    double z[NTAPS - 1];
#pragma unroll
    for (int j = 0; j < NTAPS - 1; j++) z[j] = 0.0;
    for (int64_t c0 = 0; c0 < Lcmax; c0 += SL_TILE) {
        sl_tile_load(tile, Y, q0, nrows, c0, Lcmax, lane);
        __syncthreads();
        for (int k = 0; k < SL_TILE; k++) {
            if (c0 + k < len) {
                const double v = mine[k], x = st.demean ? v - mean : v;
                const double y = z[0] + st.b[0] * x;
#pragma unroll
                for (int j = 0; j < NTAPS - 2; j++) z[j] = (z[j + 1] + x * st.b[j + 1]) - y * st.a[j + 1];
                z[NTAPS - 2] = x * st.b[NTAPS - 1] - y * st.a[NTAPS - 1];
                mine[k] = y;
            }
        }
        __syncthreads();
        if (c0 + lane < Lcmax)
            for (int j = 0; j < nrows; j++) Y[(q0 + j) * Lcmax + c0 + lane] = tile[j * SL_TILE_LD + lane];
        __syncthreads();
    }
}

template <int NTAPS>
static void sl_filter_launch(beatamd_ctx *ctx, int64_t Q, int64_t D, int64_t L, int64_t ntmax, const int32_t *nt, int64_t Lcmax,
                             const SlStage &st, double *Y)
{
    hipLaunchKernelGGL(k_trace_filter<NTAPS>, dim3((unsigned)((Q + SL_TILE - 1) / SL_TILE)), dim3(64), 0, ctx->stream, Q, D, L,
                       ntmax, nt, Lcmax, st, Y);
}

int launch_trace_filter(beatamd_ctx *ctx, int64_t Q, int64_t D, int64_t L, int64_t ntmax, const int32_t *nt, int64_t Lcmax,
                        const SlStage &st, double *Y)
{
    if (Q == 0) return BEATAMD_OK;
    BA_CHECK(st.ntaps >= SL_MIN_TAPS && st.ntaps <= SL_MAX_TAPS, BEATAMD_EINVAL, "trace_filter: a stage of %d taps (%d ... %d)",
             st.ntaps, SL_MIN_TAPS, SL_MAX_TAPS);
    BA_CHECK((Q + SL_TILE - 1) / SL_TILE < (int64_t)0x7fffffff && D >= 1 && L >= 1 && Lcmax >= L && Lcmax <= L + ntmax - 1,
             BEATAMD_EINVAL, "trace_filter: bad trace count or length");
    ScopedTimer tm(ctx, "trace_filter");
    switch (st.ntaps) {
#define SL_CASE(n) case n: sl_filter_launch<n>(ctx, Q, D, L, ntmax, nt, Lcmax, st, Y); break;
        SL_CASE(3) SL_CASE(4) SL_CASE(5) SL_CASE(6) SL_CASE(7) SL_CASE(8) SL_CASE(9) SL_CASE(10) SL_CASE(11) SL_CASE(12)
        SL_CASE(13) SL_CASE(14) SL_CASE(15) SL_CASE(16) SL_CASE(17)
#undef SL_CASE
    }
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ---- k_library_windows: one workgroup <-> one trace q of the block; its row of Y is read from HBM once (the S windows
// overlap: the re-reads are cache hits) and written S times.  Two samples a lane and one 16-byte store where the library's
// rows are 16-byte aligned (N even, the storage aligned); the reads of Y start at i0, which may be odd, and stay 8 bytes.
// i0 is clamped to [-N, Lcmax] first: a window wholly outside stays wholly outside and i0 + n cannot overflow.  The loads are
// unconditional at an index clamped into the trace (len >= 1), the zero fill is a select: no branch around a load.
__device__ __forceinline__ int64_t sl_clamp(int64_t k, int64_t len) { return k < 0 ? 0 : (k < len ? k : len - 1); }
template <bool VEC>
__global__ void __launch_bounds__(256) k_library_windows(int64_t Q, int64_t P, int64_t p0, int64_t pb, int64_t D, int64_t L,
                                                         int64_t ntmax, const int32_t *nt, int64_t Lcmax, const double *Y, int64_t S,
                                                         int64_t N, const int64_t *I0, const double *W0, double *lib)
{
#pragma clang fp contract(off)
    const int64_t q = blockIdx.x;
    if (q >= Q) return;
    const SlTrace tr = sl_trace(q, pb, D, L, nt, ntmax, Lcmax);
    const int64_t tp = tr.t * P + p0 + tr.pl;
    const double *y = Y + q * Lcmax;
    for (int64_t s = 0; s < S; s++) {
        int64_t i0 = I0[tp * S + s];
        i0 = i0 < -N ? -N : (i0 > Lcmax ? Lcmax : i0);
        const double w = W0[tp * S + s];
        double *row = lib + ((tp * D + tr.d) * S + s) * N;
        if (VEC) {
#pragma unroll 8       // the loads of eight stores in flight
            for (int64_t j = threadIdx.x; j < N / 2; j += 256) {
                const int64_t k = i0 + 2 * j;
                const double y0 = y[sl_clamp(k, tr.len)], y1 = y[sl_clamp(k + 1, tr.len)];
                double2 v;
                v.x = (k >= 0 && k < tr.len) ? y0 : 0.0;
                v.y = (k + 1 >= 0 && k + 1 < tr.len) ? y1 : 0.0;
                if (j == 0) v.x = v.x * w;
                *reinterpret_cast<double2 *>(row + 2 * j) = v;
            }
        } else {
#pragma unroll 8
            for (int64_t n = threadIdx.x; n < N; n += 256) {
                const int64_t k = i0 + n;
                const double y0 = y[sl_clamp(k, tr.len)];
                double v = (k >= 0 && k < tr.len) ? y0 : 0.0;
                if (n == 0) v = v * w;
                row[n] = v;
            }
        }
    }
}

int launch_library_windows(beatamd_ctx *ctx, int64_t T, int64_t P, int64_t p0, int64_t pb, int64_t D, int64_t L, int64_t ntmax,
                           const int32_t *nt, int64_t Lcmax, const double *Y, int64_t S, int64_t N, const int64_t *i0,
                           const double *w0, double *lib)
{
    const int64_t Q = T * pb * D;
    if (Q == 0 || S == 0 || N == 0) return BEATAMD_OK;
    BA_CHECK(Q < (int64_t)0x7fffffff && p0 >= 0 && pb >= 1 && p0 + pb <= P && L >= 1 && Lcmax >= L && Lcmax <= L + ntmax - 1 &&
                 S >= 1 && N >= 1,
             BEATAMD_EINVAL, "library_windows: bad block of patches, trace length or window");
    const bool vec = N % 2 == 0 && ((uintptr_t)lib & 15) == 0;
    ScopedTimer tm(ctx, "lib_windows");
    if (vec)
        hipLaunchKernelGGL(k_library_windows<true>, dim3((unsigned)Q), dim3(256), 0, ctx->stream, Q, P, p0, pb, D, L, ntmax, nt,
                           Lcmax, Y, S, N, i0, w0, lib);
    else
        hipLaunchKernelGGL(k_library_windows<false>, dim3((unsigned)Q), dim3(256), 0, ctx->stream, Q, P, p0, pb, D, L, ntmax, nt,
                           Lcmax, Y, S, N, i0, w0, lib);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
