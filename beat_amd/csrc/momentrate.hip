// momentrate.hip -- moment, moment magnitude and moment-rate function of every draw of a population: what the reference
// computes one point at a time with a Python loop over the patches (ffi/fault.py:284-474).  pyrocko enters the reference
// in two places, both replaced by data or a closed formula here:
//   * RectangularSource.get_moment -- the shear modulus under a patch times its area times its slip: linear in the slip,
//     so the caller hands k [P] = "moment per unit slip" of every patch (rs.get_moment at unit slip)
//   * stf.discretize_t -- the discretised source-time function, k_moment_rate below
// UNVERIFIED against pyrocko (it is not installed where this was written; both are restated from memory of its source):
//   moment_to_magnitude(M0) = log10(M0 * 1e7) / 1.5 - 10.7
//   HalfSinusoidSTF.discretize_t with exponent = 1 (BEAT's default stf_type), the rule stated at k_moment_rate
// All arithmetic is FP64 with contraction off: tests/momentrate_ref.py restates every kernel operation by operation.
#include "devmath.hpp"
#include "kernels.hpp"
#include "stf.hpp"
#include "wave.hpp"

namespace beatamd {

constexpr double MR_INDEX_MAX = 1099511627776.0;   // 2^40: a grid index beyond it flags the draw (no int64 overflow)

// ---- fault.py:317-359 get_moment / get_magnitude, :343-359 get_total_slip, :284-315 get_subfault_patch_moments
// One wavefront <-> one draw.  slip_p = sqrt(((0 + s_0^2) + s_1^2) ...) over the components in the order given (numpy's
// `slips += var ** 2`), term_p = k_p * slip_p, exactly 0 for slip_p == 0 (:309-312).  M0 = the terms summed in patch
// order, one after the other from 0.0: the order is fixed and does not depend on the batch.  (DEVIATION: the reference's
// num.array(moments).sum() is numpy's pairwise sum.)  Lanes form MAG_CHUNK terms at a time into LDS; every lane then
// adds them in order, so all lanes hold the same M0.  Mw = 0 for M0 == 0 (:338-341: `if moment`), NaN stays NaN.
constexpr int MAG_CHUNK = 256;

__global__ void __launch_bounds__(64) k_moment_magnitude(int64_t P, const double *Q, int64_t np, MrComps comps, const double *k,
                                                         double *M0, double *Mw)
{
#pragma clang fp contract(off)
    __shared__ double term[MAG_CHUNK];
    const int lane = threadIdx.x;
    const double *q = Q + (int64_t)blockIdx.x * np;
    double m0 = 0.0;
    for (int64_t p0 = 0; p0 < P; p0 += MAG_CHUNK) {
#pragma unroll
        for (int u = 0; u < MAG_CHUNK / 64; u++) {
            const int64_t p = p0 + u * 64 + lane;
            if (p < P) {
                double s2 = 0.0;
                for (int v = 0; v < comps.n; v++) {
                    const double s = q[comps.off[v] + p];
                    s2 = s2 + s * s;
                }
                const double slip = sqrt(s2);
                term[u * 64 + lane] = slip != 0.0 ? k[p] * slip : 0.0;
            }
        }
        __syncthreads();
        const int n = (int)(P - p0 < MAG_CHUNK ? P - p0 : MAG_CHUNK);
        for (int i = 0; i < n; i++) m0 = m0 + term[i];
        __syncthreads();
    }
    if (lane == 0) {
        M0[blockIdx.x] = m0;
        Mw[blockIdx.x] = m0 == 0.0 ? 0.0 : log10(m0 * 1.0e7) / 1.5 - 10.7;
    }
}

int launch_moment_magnitude(beatamd_ctx *ctx, int64_t C, int64_t P, const double *Q, int64_t np, const MrComps &comps,
                            const double *k, double *M0, double *Mw)
{
    if (C == 0) return BEATAMD_OK;
    BA_CHECK(C < (int64_t)0x7fffffff, BEATAMD_EINVAL, "magnitudes: too many draws in one call");
    ScopedTimer tm(ctx, "magnitude");
    hipLaunchKernelGGL(k_moment_magnitude, dim3((unsigned)C), dim3(64), 0, ctx->stream, P, Q, np, comps, k, M0, Mw);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ---- fault.py:413-420 (the time axis of a subfault), :461-465 (of the total).  One wavefront <-> one draw.
// Row s < nsub of spans [C, nsub + 1, 2]:   first = floor(min_p start / deltat),
//                                           count = ceil((max_p start + max_allP duration) / deltat) + 1 - first
// over the patches p of subfault s; the largest duration is the whole fault's (point["durations"].max()).  Row nsub, the
// total: first = the smallest first, count = the largest first + count less that.  DEVIATION: integer indices, a time is
// index * deltat; the reference's num.arange on floats has the same length wherever its float steps are exact.
// A draw flagged in chain_bad gets count = 0 in every row, and so does (DEVIATION: the reference would fail in arange or
// draw garbage) a draw with an onset or a duration that is not finite, a negative duration, or an index beyond 2^40 --
// that one raises ST_SPAN_BAD.  min / max are exact, so the reduction order is immaterial.
__global__ void __launch_bounds__(64) k_moment_rate_span(int64_t P, int nsub, const int32_t *sf_off, const int32_t *sf_ndip,
                                                         const int32_t *sf_nstrike, const double *st0, const int32_t *chain_bad,
                                                         const double *Q, int64_t np, int64_t dur_off, double deltat,
                                                         int64_t *spans, int *status)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x;
    const double *dur = Q + c * np + dur_off, *st = st0 + c * P;
    int64_t *sp = spans + c * (nsub + 1) * 2;
    const bool flagged = chain_bad && chain_bad[c] != 0;
    double dmax = -__builtin_inf();
    int bad = 0;
    for (int64_t p = lane; p < P; p += 64) {
        const double d = dur[p], t = st[p];
        if (!(d >= 0.0 && is_finite(d)) || !is_finite(t)) bad = 1;
        dmax = fmax(dmax, d);
    }
    dmax = wave_butterfly<OpFmax>(dmax);
    bad = __any(bad);
    int64_t tfirst = 0, tend = 0;
    bool any = false;
    for (int s = 0; s < nsub && !bad && !flagged; s++) {
        const int64_t p0 = sf_off[s], n = (int64_t)sf_ndip[s] * sf_nstrike[s];
        double lo = __builtin_inf(), hi = -__builtin_inf();
        for (int64_t p = p0 + lane; p < p0 + n; p += 64) {
            lo = fmin(lo, st[p]);
            hi = fmax(hi, st[p]);
        }
        lo = wave_butterfly<OpFmin>(lo);
        hi = wave_butterfly<OpFmax>(hi);
        const double a = floor(lo / deltat), b = ceil((hi + dmax) / deltat);
        if (!(fabs(a) <= MR_INDEX_MAX) || !(fabs(b) <= MR_INDEX_MAX)) {
            bad = 1;
            break;
        }
        const int64_t first = (int64_t)a, count = (int64_t)b + 1 - first;
        if (lane == 0) { sp[2 * s] = first; sp[2 * s + 1] = count; }
        tfirst = any ? (first < tfirst ? first : tfirst) : first;
        tend = any ? (first + count > tend ? first + count : tend) : first + count;
        any = true;
    }
    if (lane != 0) return;
    if (bad || flagged || !any) {
        for (int s = 0; s <= nsub; s++) { sp[2 * s] = 0; sp[2 * s + 1] = 0; }
        if (bad && !flagged) atomicOr(status, ST_SPAN_BAD);
    } else {
        sp[2 * nsub] = tfirst;
        sp[2 * nsub + 1] = tend - tfirst;
    }
}

int launch_moment_rate_span(beatamd_ctx *ctx, const FfiModel &m, int64_t C, const double *Q, const double *st0,
                            const int32_t *chain_bad, double deltat, int64_t *spans)
{
    if (C == 0) return BEATAMD_OK;
    BA_CHECK(C < (int64_t)0x7fffffff, BEATAMD_EINVAL, "moment_rate_spans: too many draws in one call");
    ScopedTimer tm(ctx, "mr_span");
    hipLaunchKernelGGL(k_moment_rate_span, dim3((unsigned)C), dim3(64), 0, ctx->stream, m.P, (int)m.nsub, m.d_patch_off.get(),
                       m.d_ndip.get(), m.d_nstrike.get(), st0, chain_bad, Q, m.layout.nparams, m.layout.durations_off, deltat,
                       spans, ctx->d_status);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ---- fault.py:361-443 get_subfault_patch_stfs / get_subfault_moment_rate_function.  One wavefront <-> (subfault, draw);
// the subfault's row of NT doubles lives in LDS, lanes <-> the samples of the current patch's source-time function (a
// loop where there are more than 64).  Patches are taken in patch order, a patch's samples land on distinct cells: no
// floating-point atomics, and the sum in every cell has the reference's order.
//
// The half-sinusoid of a patch (pyrocko HalfSinusoidSTF.discretize_t, exponent 1, anchor -1 as base.py:1013 sets it, so
// t0 = start and t1 = start + duration; UNVERIFIED, see the head of the file):
//     k0 = rint(t0 / deltat), k1 = rint(t1 / deltat) (half to even, Python's round), nt = k1 - k0 + 1
//     nt == 1:  a = [1]
//     else      e_i = max(t0, min(t1, k0 deltat + (i - 0.5) deltat)), i = 0 .. nt
//               F_i = -cos((e_i - t0) (pi / duration)),  a_i = F_{i+1} - F_i,  a_i = a_i / S
//     S, the FIXED normalisation order: lane l adds a_l, a_{l+64}, a_{l+128} ... one after the other from 0.0; the 64 lane
//     sums v are then folded v[l] = v[l] + v[l + 32] (l < 32), + v[l + 16] (l < 16), ... + v[l + 1] (l = 0).  (DEVIATION:
//     the reference's num.sum is numpy's pairwise sum.)
//     row[k0 - kbase + i] += a_i * m,  m = k_p * slip_p as in k_moment_magnitude (fault.py:412: uparr, uperp)
// The value is a moment per sample, not divided by deltat, as in the reference.
//
// A draw whose span (spans row nsub) has count 0 -- chain_bad and the other cases of k_moment_rate_span -- gets NaN rows.
// A draw whose span does not lie within [kbase, kbase + NT) gets NaN rows and raises ST_SPAN_OOB.  Every cell index is
// checked against the row before it is used: nothing is written out of bounds.  (mr_amplitude: stf.hpp, shared with the
// library producer's k_stf_table.)
__global__ void __launch_bounds__(64) k_moment_rate(int64_t P, int nsub, const int32_t *sf_off, const int32_t *sf_ndip,
                                                    const int32_t *sf_nstrike, const double *st0, const double *Q, int64_t np,
                                                    int64_t dur_off, MrComps comps, const double *k, double deltat,
                                                    const int64_t *spans, int64_t kbase, int64_t NT, double *out, int *status)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double mr_row[];
    const int lane = threadIdx.x, s = blockIdx.x;
    const int64_t c = blockIdx.y;
    const double *q = Q + c * np, *st = st0 + c * P;
    const int64_t *tot = spans + (c * (nsub + 1) + nsub) * 2;
    double *row = out + (c * (nsub + 1) + s) * NT;
    const int64_t tfirst = tot[0], tcount = tot[1];
    const bool fits = tcount > 0 && tfirst >= kbase && tfirst + tcount <= kbase + NT;
    if (!fits) {
        for (int64_t j = lane; j < NT; j += 64) row[j] = __builtin_nan("");
        if (tcount > 0 && lane == 0 && s == 0) atomicOr(status, ST_SPAN_OOB);
        return;
    }
    for (int64_t j = lane; j < NT; j += 64) mr_row[j] = 0.0;
    __syncthreads();
    const int64_t p0 = sf_off[s], n = (int64_t)sf_ndip[s] * sf_nstrike[s];
    for (int64_t p = p0; p < p0 + n; p++) {
        double s2 = 0.0;
        for (int v = 0; v < comps.n; v++) {
            const double sl = q[comps.off[v] + p];
            s2 = s2 + sl * sl;
        }
        const double slip = sqrt(s2);
        const double m = slip != 0.0 ? k[p] * slip : 0.0;
        const double t0 = st[p], d = q[dur_off + p], t1 = t0 + d;
        const double r0 = rint(t0 / deltat), r1 = rint(t1 / deltat);
        const int64_t k0 = (int64_t)r0, nt = (int64_t)r1 - k0 + 1, base = k0 - kbase;
        if (nt < 1 || base < 0 || base + nt > NT) continue;      // (cannot happen inside a span that fits; uniform)
        if (nt == 1) {
            if (lane == 0) mr_row[base] = mr_row[base] + 1.0 * m;
        } else {
            const double tmin = r0 * deltat, w = 3.14159265358979323846 / d;
            double a0 = 0.0, part = 0.0;
            for (int64_t i = lane; i < nt; i += 64) {
                const double a = mr_amplitude(i, tmin, t0, t1, w, deltat);
                if (i == lane) a0 = a;
                part = part + a;
            }
            part = wave_butterfly<OpAdd>(part);
            for (int64_t i = lane; i < nt; i += 64) {
                double a = i == lane ? a0 : mr_amplitude(i, tmin, t0, t1, w, deltat);
                a = a / part;
                mr_row[base + i] = mr_row[base + i] + a * m;
            }
        }
        __syncthreads();
    }
    for (int64_t j = lane; j < NT; j += 64) row[j] = mr_row[j];
}

// fault.py:466-472: the total = zeros, += every subfault's row in subfault order (row nsub of a draw)
__global__ void __launch_bounds__(256) k_moment_rate_total(int64_t C, int nsub, int64_t NT, double *out)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C * NT) return;
    const int64_t c = i / NT, j = i - c * NT;
    double *rows = out + c * (nsub + 1) * NT + j;
    double t = 0.0;
    for (int s = 0; s < nsub; s++) t = t + rows[s * NT];
    rows[nsub * NT] = t;
}

int launch_moment_rate(beatamd_ctx *ctx, const FfiModel &m, int64_t C, const double *Q, const double *st0, const MrComps &comps,
                       const double *k, double deltat, const int64_t *spans, int64_t kbase, int64_t NT, double *out)
{
    BA_CHECK(NT >= 1 && NT <= MR_NT_MAX, BEATAMD_EINVAL, "moment_rates: %lld samples per row (1 ... %d: the row lives in LDS)",
             (long long)NT, MR_NT_MAX);
    if (C == 0) return BEATAMD_OK;
    BA_CHECK(m.nsub >= 1 && C <= 65535 * (int64_t)1024 && (C * NT + 255) / 256 < (int64_t)0x7fffffff, BEATAMD_EINVAL,
             "moment_rates: too many draws or samples in one call");
    const size_t lds = (size_t)NT * sizeof(double);
    if (lds > 64 * 1024)
        BA_HIP(hipFuncSetAttribute((const void *)k_moment_rate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ScopedTimer tm(ctx, "mr_rate");
    // (the grid's y extent is 65535: the draws go in slabs)
    for (int64_t c0 = 0; c0 < C; c0 += 65535) {
        const int64_t nc = std::min<int64_t>(65535, C - c0);
        hipLaunchKernelGGL(k_moment_rate, dim3((unsigned)m.nsub, (unsigned)nc), dim3(64), lds, ctx->stream, m.P, (int)m.nsub,
                           m.d_patch_off.get(), m.d_ndip.get(), m.d_nstrike.get(), st0 + c0 * m.P, Q + c0 * m.layout.nparams,
                           m.layout.nparams, m.layout.durations_off, comps, k, deltat, spans + c0 * (m.nsub + 1) * 2, kbase, NT,
                           out + c0 * (m.nsub + 1) * NT, ctx->d_status);
        BA_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_moment_rate_total, dim3((unsigned)((C * NT + 255) / 256)), dim3(256), 0, ctx->stream, C, (int)m.nsub, NT,
                       out);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
