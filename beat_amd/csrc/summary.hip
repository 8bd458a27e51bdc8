// summary.hip -- posterior diagnostics of a whole stage population: variance reductions from the cached misfits,
// standardized residuals, and running moments of an ensemble of synthetics.  The forward model and the quadratic
// forms are the likelihood's own kernels (capi.cpp); what is here is the arithmetic the reference does after them.
#include "kernels.hpp"

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

}  // namespace beatamd
