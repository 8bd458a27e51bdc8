// spectrum.hip -- amplitude spectra of batches of real traces: the spectrum domain of a seismic wavemap
// (WaveformFitConfig.domain = "spectrum", heart.py:526).  Per row what the reference's geometry mode computes one trace at
// a time in Python (heart.fft_transforms, heart.py:4091-4155, outmode "array"; pytensorf.SeisSynthesizer,
// pytensorf.py:294-311; WaveformMapping.prepare_data, heart.py:3086-3095):
//     spec(y) = abs(rfft(y, ntrans))[lo:hi],   ntrans = nextpow2(len(y)) = 2^ceil(log2 N)
// (pyrocko.trace.nextpow2 is restated from memory: pyrocko is not installed where this was written), and optionally the
// residual data_spec[r mod T] - spec(x_r) that the misfit kernels consume, so that the spectra never travel.
//
// ALGORITHM (FP64 throughout, contraction off: every product and sum below is one rounded operation).
//   1. pack: z[j] = x[2j] + i x[2j+1], j < n2 = ntrans / 2; samples at index >= N are zeros that are never read from memory
//   2. complex forward FFT of the n2 points in LDS: Stockham auto-sort radix-2 stages, in place -- a pass reads all it needs
//      into registers, a barrier, then it writes (a Stockham stage is not in place by itself; the registers are the second
//      buffer).  The stage of span Ns (1, 2, 4, .. n2/2), butterfly j < n2/2, k = j mod Ns:
//          a = in[j]; b = in[j + n2/2]; w = W[k * (n2 / Ns)]
//          t.re = b.re*w.re - b.im*w.im;  t.im = b.re*w.im + b.im*w.re
//          out[(j - k)*2 + k] = a + t;  out[(j - k)*2 + k + Ns] = a - t
//      Two consecutive stages (Ns, 2 Ns) run as one pass over LDS: the thread that owns q < n2/4 computes the butterflies
//      q and q + n2/4 of the first stage and, from their four results held in registers, the two butterflies of the second
//      stage that consume exactly those.  The arithmetic is that of the two radix-2 stages, bit for bit; only the LDS
//      round trip between them is saved.  An odd stage count runs one single stage first.  A thread holds at most
//      SPEC_PER_THREAD = 4 quads (16 complex results) of a pass.
//   3. untangle, for the bins lo <= k < hi only (zr, zi = Z[k]; zr', zi' = Z[n2 - k]):
//          k == 0:  X = zr + zi           k == n2 (Nyquist):  X = zr - zi           (both real: amplitude |X|)
//          else  er = 0.5*(zr + zr'); ei = 0.5*(zi - zi'); or = 0.5*(zi + zi'); oi = 0.5*(zr' - zr); w = W[k]
//                xr = er + (or*w.re - oi*w.im);  xi = ei + (or*w.im + oi*w.re)
//      amplitude = sqrt(xr*xr + xi*xi) (not hypot: overflow is no concern at seismogram magnitudes, and sqrt of the
//      rounded sum of squares is within 1.5 ulp of the amplitude)
//   4. out[r, k - lo] = amplitude, or data_spec[r mod T, k - lo] - amplitude (one subtraction more, nothing else differs)
// TWIDDLES: a table W[k] = exp(-2 pi i k / ntrans), k < ntrans/2, computed on the host (spectrum_twiddles: cosl / sinl in
// extended precision, rounded once to double) and uploaded once per ntrans and context; stages and the untangling pass read
// it from global memory (it is at most 64 KiB and shared by every row: it stays in L2).
// A row's result is a function of its samples, N, ntrans, lo, hi alone: no sum crosses rows, the operation order above does
// not depend on which thread runs a butterfly, so R, the row's position and the launch shape cannot change a bit.  An
// all-zero row gives exact zeros (every product is a zero, sqrt(0) = 0).
//
// LAUNCH SHAPES.  TEAM threads own one row; a workgroup of 256 threads holds 256 / TEAM rows.
//   ntrans <= 512: TEAM = 64, one wavefront per trace, four traces per workgroup (config 4's 120-sample traces, ntrans 128:
//                  2 KiB of LDS per trace)
//   ntrans >= 1024: TEAM = 256, one workgroup per trace
// LDS: n2 complex doubles per row = 8 * ntrans bytes: 1 KiB per trace (4 KiB per workgroup) at ntrans 128, 32 KiB at 4096
// (five workgroups per CU), 64 KiB at 8192 (two).  Power-of-two strides of 16-byte elements: the reads of a pass are
// contiguous per lane group (stride 1 in q); the writes of the early stages (Ns < 16) are strided by 2 Ns or 4 Ns elements
// and conflict.  Not padded: profiles/spectrum_timing.json has the measured rate, DESIGN.md what bounds it.
#include <cmath>

#include "kernels.hpp"

namespace beatamd {

constexpr int SPEC_PER_THREAD = 4;   // butterflies / quads of a pass a thread holds in registers (k_amp_spectrum)

struct alignas(16) cplx {   // (16-byte elements: one ds_read_b128 / ds_write_b128 each; the row buffers start 16-byte aligned)
    double re, im;
};

__device__ __forceinline__ cplx c_mul(cplx b, cplx w)
{
#pragma clang fp contract(off)
    cplx t;
    t.re = b.re * w.re - b.im * w.im;
    t.im = b.re * w.im + b.im * w.re;
    return t;
}
__device__ __forceinline__ cplx c_add(cplx a, cplx b) { return cplx{a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cplx c_sub(cplx a, cplx b) { return cplx{a.re - b.re, a.im - b.im}; }

// rows of X [R, N] (row stride xs) -> out [R, M = hi - lo]; dynamic LDS: (256 / TEAM) * n2 complex doubles
template <int TEAM>
__global__ void __launch_bounds__(256) k_amp_spectrum(int64_t R, int64_t N, int64_t xs, int ntrans, int lo, int hi, const double *X,
                                                      const cplx *W, const double *data_spec, int64_t T, double *out)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) cplx lds_spec[];
    const int n2 = ntrans >> 1;
    const int team = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
    const int64_t r = (int64_t)blockIdx.x * (256 / TEAM) + team;
    const bool live = r < R;   // (a team without a row keeps pace with the barriers and touches no global memory)
    cplx *buf = lds_spec + (size_t)team * n2;

    // 1. pack
    if (live) {
        const double *x = X + r * xs;
        for (int j = lane; j < n2; j += TEAM) {
            const int64_t i0 = 2 * (int64_t)j;
            cplx z;
            z.re = i0 < N ? x[i0] : 0.0;
            z.im = i0 + 1 < N ? x[i0 + 1] : 0.0;
            buf[j] = z;
        }
    }
    __syncthreads();

    // 2. the stages, in place: a pass reads everything it needs into registers, barrier, writes its results, barrier.  A
    // thread owns at most SPEC_PER_THREAD butterflies of the single stage / quads of a double stage (n2 <= 4096, TEAM
    // threads: n2 / 2 / TEAM <= 4 where the stage count is odd, n2 / 4 / TEAM <= 4)
    const int half = n2 >> 1, quarter = n2 >> 2;
    int Ns = 1;
    int nstage = 0;
    for (int m = n2; m > 1; m >>= 1) nstage++;
    if (nstage & 1) {   // one single stage (Ns = 1: k = 0, w = W[0] = 1)
        cplx c[SPEC_PER_THREAD][2];
#pragma unroll
        for (int u = 0; u < SPEC_PER_THREAD; u++) {
            const int j = lane + u * TEAM;
            if (live && j < half) {
                const cplx a = buf[j], t = c_mul(buf[j + half], W[0]);
                c[u][0] = c_add(a, t);
                c[u][1] = c_sub(a, t);
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < SPEC_PER_THREAD; u++) {
            const int j = lane + u * TEAM;
            if (live && j < half) {
                buf[2 * j] = c[u][0];
                buf[2 * j + 1] = c[u][1];
            }
        }
        __syncthreads();
        Ns = 2;
    }
    for (; Ns < n2; Ns <<= 2) {   // stages Ns and 2 Ns in one pass
        const int tstep = n2 / Ns;   // table stride of the first stage; the second's is half of it
        cplx c[SPEC_PER_THREAD][4];
#pragma unroll
        for (int u = 0; u < SPEC_PER_THREAD; u++) {
            const int q = lane + u * TEAM;
            if (live && q < quarter) {
                const int k = q & (Ns - 1);
                const cplx w1 = W[(size_t)k * tstep];
                const cplx x0 = buf[q], x1 = buf[q + quarter];
                const cplx t2 = c_mul(buf[q + half], w1), t3 = c_mul(buf[q + half + quarter], w1);
                const cplx a0 = c_add(x0, t2), a1 = c_sub(x0, t2);   // first stage, butterfly q: at p, p + Ns
                const cplx b0 = c_add(x1, t3), b1 = c_sub(x1, t3);   // butterfly q + n2/4: at p + n2/2, p + Ns + n2/2
                const cplx u0 = c_mul(b0, W[(size_t)k * (tstep >> 1)]);            // second stage, butterfly p (k' = k)
                const cplx u1 = c_mul(b1, W[(size_t)(k + Ns) * (tstep >> 1)]);     // butterfly p + Ns (k' = k + Ns)
                c[u][0] = c_add(a0, u0);
                c[u][1] = c_add(a1, u1);
                c[u][2] = c_sub(a0, u0);
                c[u][3] = c_sub(a1, u1);
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < SPEC_PER_THREAD; u++) {
            const int q = lane + u * TEAM;
            if (live && q < quarter) {
                const int k = q & (Ns - 1);
                const int o = ((q - k) << 2) + k;
                buf[o] = c[u][0];
                buf[o + Ns] = c[u][1];
                buf[o + 2 * Ns] = c[u][2];
                buf[o + 3 * Ns] = c[u][3];
            }
        }
        __syncthreads();
    }
    const cplx *in = buf;

    // 3., 4. untangle the bins asked for
    if (!live) return;
    const int M = hi - lo;
    double *o = out + r * M;
    const double *d = data_spec ? data_spec + (r % T) * M : nullptr;
    for (int i = lane; i < M; i += TEAM) {
        const int k = lo + i;
        double amp;
        if (k == 0 || k == n2) {
            const cplx z = in[0];
            amp = fabs(k == 0 ? z.re + z.im : z.re - z.im);
        } else {
            const cplx z = in[k], zc = in[n2 - k], w = W[k];
            const double er = 0.5 * (z.re + zc.re), ei = 0.5 * (z.im - zc.im);
            const double orr = 0.5 * (z.im + zc.im), oi = 0.5 * (zc.re - z.re);
            const double xr = er + (orr * w.re - oi * w.im);
            const double xi = ei + (orr * w.im + oi * w.re);
            amp = sqrt(xr * xr + xi * xi);
        }
        o[i] = d ? d[i] - amp : amp;
    }
}

// the table of one transform length, made on first use and kept by the context (never inside a graph capture: the entry
// points that add a spectrum wavemap or transform a batch call this before anything is captured)
int spectrum_twiddles(beatamd_ctx *ctx, int64_t ntrans, const double **W)
{
    BA_CHECK(ntrans >= SPEC_NTRANS_MIN && ntrans <= SPEC_NTRANS_MAX && (ntrans & (ntrans - 1)) == 0, BEATAMD_EINVAL,
             "amp_spectrum: transform length %lld is not a power of two in [%d, %d]", (long long)ntrans, SPEC_NTRANS_MIN,
             SPEC_NTRANS_MAX);
    auto it = ctx->twiddles.find(ntrans);
    if (it == ctx->twiddles.end()) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        BA_HIP(hipStreamIsCapturing(ctx->stream, &cap));
        BA_CHECK(cap == hipStreamCaptureStatusNone, BEATAMD_EINVAL,
                 "amp_spectrum: the twiddle table of length %lld is missing inside a graph capture", (long long)ntrans);
        const int64_t n2 = ntrans / 2;
        std::vector<double> h((size_t)(2 * n2));
        const long double step = -2.0L * 3.141592653589793238462643383279502884L / (long double)ntrans;
        for (int64_t k = 0; k < n2; k++) {
            h[(size_t)(2 * k)] = (double)cosl(step * (long double)k);
            h[(size_t)(2 * k + 1)] = (double)sinl(step * (long double)k);
        }
        if (n2 >= 2) {   // exact where the exact value is representable
            h[(size_t)n2] = 0.0;
            h[(size_t)n2 + 1] = -1.0;
        }
        DevMem<double> d;
        BA_TRY(d.alloc_copy(ctx, h.data(), h.size()));
        it = ctx->twiddles.emplace(ntrans, std::move(d)).first;
    }
    *W = it->second.get();
    return BEATAMD_OK;
}

int spectrum_check_band(int64_t N, int64_t ntrans, int64_t lo, int64_t hi)
{
    BA_CHECK(ntrans >= SPEC_NTRANS_MIN && ntrans <= SPEC_NTRANS_MAX && (ntrans & (ntrans - 1)) == 0, BEATAMD_EINVAL,
             "amp_spectrum: transform length %lld is not a power of two in [%d, %d]", (long long)ntrans, SPEC_NTRANS_MIN,
             SPEC_NTRANS_MAX);
    BA_CHECK(N >= 1 && N <= ntrans, BEATAMD_EINVAL, "amp_spectrum: %lld samples do not fit a transform of %lld",
             (long long)N, (long long)ntrans);
    BA_CHECK(0 <= lo && lo < hi && hi <= ntrans / 2 + 1, BEATAMD_EINVAL,
             "amp_spectrum: spectrum band [%lld, %lld) outside the %lld bins of a transform of %lld", (long long)lo,
             (long long)hi, (long long)(ntrans / 2 + 1), (long long)ntrans);
    return BEATAMD_OK;
}

int launch_amp_spectrum(beatamd_ctx *ctx, int64_t R, int64_t N, int64_t xs, int64_t ntrans, int64_t lo, int64_t hi,
                        const double *X, const double *data_spec, int64_t T, double *out)
{
    BA_TRY(spectrum_check_band(N, ntrans, lo, hi));
    BA_CHECK(xs >= N && (!data_spec || T > 0), BEATAMD_EINVAL, "amp_spectrum: bad row stride or dataset count");
    if (R == 0) return BEATAMD_OK;
    const double *W;
    BA_TRY(spectrum_twiddles(ctx, ntrans, &W));
    // what a thread holds of a pass: quads n2 / 4 / TEAM, butterflies of the single stage n2 / 2 / TEAM (odd stage counts:
    // n2 <= 2048 in a workgroup, n2 <= 128 in a wavefront)
    static_assert(SPEC_NTRANS_MAX / 2 / 4 / 256 <= SPEC_PER_THREAD && SPEC_NTRANS_MAX / 4 / 2 / 256 <= SPEC_PER_THREAD &&
                      SPEC_WAVE_NTRANS / 2 / 4 / 64 <= SPEC_PER_THREAD, "k_amp_spectrum: a pass does not fit a thread's registers");
    const bool wave = ntrans <= SPEC_WAVE_NTRANS;
    const int rows_per_wg = wave ? 4 : 1;
    const int64_t nwg = (R + rows_per_wg - 1) / rows_per_wg;
    BA_CHECK(nwg < (int64_t)0x7fffffff, BEATAMD_EINVAL, "amp_spectrum: too many rows in one call");
    const size_t lds = (size_t)rows_per_wg * (size_t)(ntrans / 2) * sizeof(cplx);
    ScopedTimer tm(ctx, "amp_spectrum");
    if (wave) {
        hipLaunchKernelGGL(k_amp_spectrum<64>, dim3((unsigned)nwg), dim3(256), lds, ctx->stream, R, N, xs, (int)ntrans, (int)lo,
                           (int)hi, X, (const cplx *)W, data_spec, T, out);
    } else {
        if (lds > 64 * 1024)
            BA_HIP(hipFuncSetAttribute((const void *)k_amp_spectrum<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_amp_spectrum<256>, dim3((unsigned)nwg), dim3(256), lds, ctx->stream, R, N, xs, (int)ntrans, (int)lo,
                           (int)hi, X, (const cplx *)W, data_spec, T, out);
    }
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
