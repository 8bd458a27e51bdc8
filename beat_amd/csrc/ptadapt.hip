// ptadapt.hip -- the proposal covariance of every temperature of a parallel-tempering run, learned while the chains run.
//
// The reference's PT workers re-learn their MultivariateNormalProposal from their own trace every buffer_size samples
// (sample_pt_chain, beat/sampler/pt.py:758-761; _iter_sample, beat/sampler/base.py:363-393; BaseChain.get_sample_covariance,
// beat/backend.py:249-268; calc_sample_covariance, beat/covariance.py:865-909: the likelihood-weighted numpy.cov(...,
// aweights=, bias=False)).  A window of buffer_size x replicas states per temperature cannot be held for ~10^3 parameters,
// so its weighted moments are accumulated after every step instead:
//
//   state of a group (GM_HDR + n + n*n doubles):  m, S0, Sw2, count, nbad, 3 spare | S1 [n] | S2 [n, n] (lower triangle)
//
//   update with the R rows of the group:  m' = max(m, max_r like_r),  s = exp(m - m'),  w_r = exp(like_r - m'),
//       y_r = x_r - ref,   S0 = S0 s + sum w_r,   Sw2 = Sw2 s^2 + sum w_r^2,   S1 = S1 s + sum w_r y_r,
//       S2 = S2 s + sum w_r y_r y_r^T          (the weights of covariance.py:889-891 up to a factor that cancels)
//   a row with a non-finite like or state counts in nbad and adds nothing.
//
//   k_gm_reset / k_gm_ref   a window opens: empty state, ref = mean of the group's rows
//   k_gm_weights   one workgroup per group: row flags, m', the weights, the header
//   k_gm_s1        S1, one thread per parameter, rows in order
//   k_gm_s2        S2 on the FP64 matrix cores (v_mfma_f64_16x16x4_f64, the operand layout of gemm.hip): a workgroup owns
//                  one 64 x 64 tile of the lower triangle of one group, walks the R rows in steps of 16 through a double-
//                  buffered LDS stage and folds the rescale into the read-modify-write of its tile
//   k_gm_check / k_gm_cov / (potrf_lower of chol.hip) / k_gm_store      mean, covariance, upper factor, flags
//
// Every accumulator entry is owned by one thread of one workgroup whose geometry is fixed, and sees the rows of its group in
// index order: the sums depend on (group, replica, order of the calls) alone.  No atomics.
#include "devmath.hpp"
#include "kernels.hpp"
#include "wave.hpp"

namespace beatamd {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int GM_TB = 256;
constexpr int GM_T = 64, GM_KS = 16, GM_P = GM_KS + 1;   // S2 tile edge, rows per LDS stage, LDS pitch

__global__ void __launch_bounds__(GM_TB) k_gm_reset(double *state, int64_t stride)
{
    double *st = state + (int64_t)blockIdx.y * stride;
    const int64_t i = (int64_t)blockIdx.x * GM_TB + threadIdx.x;
    if (i < stride) st[i] = (i == 0) ? -INFINITY : 0.0;
}

// ref[g, j] = mean over the R rows of group g, summed in replica order (the reference point of a window that opens)
__global__ void __launch_bounds__(GM_TB) k_gm_ref(const double *Q, int64_t R, int64_t n, double *ref)
{
    const int64_t g = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * GM_TB + threadIdx.x;
    if (j >= n) return;
    double acc = 0.0;
    for (int64_t r = 0; r < R; r++) acc += Q[(g * R + r) * n + j];
    ref[g * n + j] = acc / (double)R;
}

__global__ void __launch_bounds__(GM_TB) k_gm_weights(const double *Q, const double *like, int64_t lstride, int64_t R, int64_t n,
                                                      double *state, int64_t stride, double *w, double *scale)
{
    __shared__ double wl[GM_MAX_R];
    __shared__ double red[GM_TB];
    const int64_t g = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double *st = state + g * stride;
    // a row is used iff its like and every component of its state are finite; wl[r] = like or NaN
    for (int64_t r = wave; r < R; r += GM_TB / 64) {
        const double *x = Q + (g * R + r) * n;
        const double lk = like[(g * R + r) * lstride];
        int bad = is_finite(lk) ? 0 : 1;
        for (int64_t j = lane; j < n; j += 64) bad |= is_finite(x[j]) ? 0 : 1;
        bad = __any(bad);
        if (lane == 0) wl[r] = bad ? NAN : lk;
    }
    __syncthreads();
    double mx = -INFINITY;
    for (int64_t r = tid; r < R; r += GM_TB) {
        const double v = wl[r];
        if (v == v) mx = fmax(mx, v);
    }
    red[tid] = mx;
    __syncthreads();
    for (int h = GM_TB / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = fmax(red[tid], red[tid + h]);
        __syncthreads();
    }
    const double m_old = st[0];
    const double m_new = fmax(m_old, red[0]);
    double sw = 0.0, sw2 = 0.0, cnt = 0.0, nb = 0.0;
    for (int64_t r = tid; r < R; r += GM_TB) {
        const double v = wl[r];
        double wr = 0.0;
        if (v == v) {
            wr = exp(v - m_new);
            sw += wr;
            sw2 += wr * wr;
            cnt += 1.0;
        } else {
            nb += 1.0;
        }
        w[g * R + r] = wr;
    }
    sw = block_sum_ldstree<GM_TB>(sw, red);
    sw2 = block_sum_ldstree<GM_TB>(sw2, red);
    cnt = block_sum_ldstree<GM_TB>(cnt, red);
    nb = block_sum_ldstree<GM_TB>(nb, red);
    if (tid == 0) {
        // (nothing finite so far: m stays -inf and there is nothing to rescale)
        const double s = (m_new == -INFINITY) ? 1.0 : exp(m_old - m_new);
        st[0] = m_new;
        st[1] = st[1] * s + sw;
        st[2] = st[2] * (s * s) + sw2;
        st[3] += cnt;
        st[4] += nb;
        scale[g] = s;
    }
}

__global__ void __launch_bounds__(GM_TB) k_gm_s1(const double *Q, const double *ref, const double *w, const double *scale,
                                                 int64_t R, int64_t n, double *state, int64_t stride)
{
    const int64_t g = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * GM_TB + threadIdx.x;
    if (j >= n) return;
    const double rf = ref[g * n + j];
    double acc = 0.0;
    for (int64_t r = 0; r < R; r++) {
        const double wr = w[g * R + r];
        if (wr != 0.0) acc = fma(wr, Q[(g * R + r) * n + j] - rf, acc);
    }
    double *S1 = state + g * stride + GM_HDR;
    S1[j] = S1[j] * scale[g] + acc;
}

// S2[i, j] = S2[i, j] * s + sum_r (w_r y_ri) y_rj for one 64 x 64 tile (ib, jb <= ib) of one group.  4 wavefronts, each 16
// rows x 64 columns = four 16 x 16 accumulators; A operand (rows i) carries the weight.  A row with weight 0 is staged
// as zeros on both sides (its state may be non-finite).
__global__ void __launch_bounds__(GM_TB) k_gm_s2(const double *Q, const double *ref, const double *w, const double *scale,
                                                 int64_t R, int64_t n, double *state, int64_t stride)
{
    constexpr int NJ = GM_T / 16;
    __shared__ double As[2][GM_T * GM_P];
    __shared__ double Bs[2][GM_T * GM_P];
    const int64_t g = blockIdx.y;
    // tile t of the lower triangle in row-major order: ib (ib + 1) / 2 + jb
    int ib = 0;
    {
        int t = (int)blockIdx.x;
        while (t >= ib + 1) { t -= ib + 1; ib++; }
    }
    const int jb = (int)blockIdx.x - ib * (ib + 1) / 2;
    const bool diag = ib == jb;
    const int64_t i0 = (int64_t)ib * GM_T, j0 = (int64_t)jb * GM_T;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const double *Qg = Q + g * R * n, *wg = w + g * R, *rg = ref + g * n;

    // stage [16 rows x 64 columns] of each side: thread -> row kr, 4 consecutive columns from c4
    const int kr = tid >> 4, c4 = (tid & 15) * 4;
    double ra[4], rb[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        ra[e] = (i0 + c4 + e < n) ? rg[i0 + c4 + e] : 0.0;
        rb[e] = (j0 + c4 + e < n) ? rg[j0 + c4 + e] : 0.0;
    }
    double av[4], bv[4];
    auto load_stage = [&](int64_t k0) {
        const int64_t r = k0 + kr;
        const double wr = (r < R) ? wg[r] : 0.0;
        const double *x = Qg + r * n;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const bool oka = wr != 0.0 && i0 + c4 + e < n, okb = wr != 0.0 && j0 + c4 + e < n;
            av[e] = oka ? wr * (x[i0 + c4 + e] - ra[e]) : 0.0;
            bv[e] = okb ? x[j0 + c4 + e] - rb[e] : 0.0;
        }
    };
    v4f64 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) acc[j] = v4f64{0.0, 0.0, 0.0, 0.0};

    load_stage(0);
    int buf = 0;
    for (int64_t k0 = 0; k0 < R; k0 += GM_KS) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            As[buf][(c4 + e) * GM_P + kr] = av[e];
            Bs[buf][(c4 + e) * GM_P + kr] = bv[e];
        }
        __syncthreads();
        if (k0 + GM_KS < R) load_stage(k0 + GM_KS);
#pragma unroll
        for (int kk = 0; kk < GM_KS / 4; kk++) {
            const int kcol = kk * 4 + (lane >> 4);
            const double aop = As[buf][(wave * 16 + (lane & 15)) * GM_P + kcol];
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                if (diag && j > wave) continue;   // a 16 x 16 block above the diagonal: never stored
                const double bop = Bs[buf][(j * 16 + (lane & 15)) * GM_P + kcol];
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop, bop, acc[j], 0, 0, 0);
            }
        }
        buf ^= 1;
    }
    // reg r of lane l -> row (l >> 4) + 4r, column l & 15 of the wave's 16 x 16 block j
    const double s = scale[g];
    double *S2 = state + g * stride + GM_HDR + n;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int64_t row = i0 + wave * 16 + (lane >> 4) + 4 * r;
        if (row >= n) continue;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int64_t col = j0 + j * 16 + (lane & 15);
            if (col > row) continue;   // (col <= row < n)
            double *p = S2 + row * n + col;
            *p = *p * s + acc[j][r];
        }
    }
}

int launch_group_moments_reset(beatamd_ctx *ctx, int64_t G, int64_t n, double *state, int64_t R, const double *Q, double *ref)
{
    const int64_t stride = group_moments_stride(n);
    const dim3 grid((unsigned)((stride + GM_TB - 1) / GM_TB), (unsigned)G);
    hipLaunchKernelGGL(k_gm_reset, grid, dim3(GM_TB), 0, ctx->stream, state, stride);
    if (ref)
        hipLaunchKernelGGL(k_gm_ref, dim3((unsigned)((n + GM_TB - 1) / GM_TB), (unsigned)G), dim3(GM_TB), 0, ctx->stream, Q, R, n,
                           ref);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_group_moments_update(beatamd_ctx *ctx, int64_t G, int64_t R, int64_t n, const double *Q, const double *like,
                                int64_t like_stride, const double *ref, double *state)
{
    const int64_t stride = group_moments_stride(n);
    double *w, *scale;
    BA_TRY(ctx->scratch(SL_GM_W, (size_t)G * R, &w));
    BA_TRY(ctx->scratch(SL_GM_SCALE, (size_t)G, &scale));
    ScopedTimer tm(ctx, "group_moments");
    hipLaunchKernelGGL(k_gm_weights, dim3((unsigned)G), dim3(GM_TB), 0, ctx->stream, Q, like, like_stride, R, n, state, stride,
                       w, scale);
    hipLaunchKernelGGL(k_gm_s1, dim3((unsigned)((n + GM_TB - 1) / GM_TB), (unsigned)G), dim3(GM_TB), 0, ctx->stream, Q, ref,
                       (const double *)w, (const double *)scale, R, n, state, stride);
    const int64_t nt = (n + GM_T - 1) / GM_T;
    hipLaunchKernelGGL(k_gm_s2, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)G), dim3(GM_TB), 0, ctx->stream, Q, ref,
                       (const double *)w, (const double *)scale, R, n, state, stride);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ---- finish: mu = S1 / S0, fact = 1 - Sw2 / S0^2, cov = (S2 / S0 - mu mu^T) / fact  (numpy.cov with normalised aweights,
// bias=False), symmetrised by copy
__device__ __forceinline__ double gm_cov_entry(const double *st, int64_t n, int64_t i, int64_t j, double S0, double fact)
{
    const double *S1 = st + GM_HDR, *S2 = S1 + n;
    const int64_t hi = i > j ? i : j, lo = i > j ? j : i;
    return (S2[hi * n + lo] / S0 - (S1[hi] / S0) * (S1[lo] / S0)) / fact;
}

// bad[g] = 1: fact <= 0, rows that were not finite, or a moment / covariance entry that is not finite
__global__ void __launch_bounds__(GM_TB) k_gm_check(const double *state, int64_t stride, int64_t n, int32_t *bad)
{
    __shared__ int any;
    const double *st = state + (int64_t)blockIdx.x * stride;
    const double S0 = st[1], fact = 1.0 - st[2] / (S0 * S0);
    if (threadIdx.x == 0) any = (!is_finite(st[0]) || !is_finite(S0) || !(fact > 0.0) || st[4] > 0.0) ? 1 : 0;
    __syncthreads();
    int mine = 0;
    for (int64_t e = threadIdx.x; e < n * n; e += GM_TB) {
        const int64_t i = e / n, j = e - i * n;
        if (j <= i && !is_finite(gm_cov_entry(st, n, i, j, S0, fact))) mine = 1;
    }
    if (mine) any = 1;   // (every writer stores the same value)
    __syncthreads();
    if (threadIdx.x == 0) bad[blockIdx.x] = any;
}

// A [G][np][np] = cov inside n x n (identity for a group flagged bad), identity in the padding; cov_out (nullable) [G][n][n]
__global__ void __launch_bounds__(GM_TB) k_gm_cov(const double *state, int64_t stride, int64_t n, int64_t np,
                                                  const int32_t *bad, double *A, double *cov_out)
{
    const int64_t g = blockIdx.y;
    const int64_t idx = (int64_t)blockIdx.x * GM_TB + threadIdx.x;
    if (idx >= np * np) return;
    const int64_t i = idx / np, j = idx - i * np;
    const double *st = state + g * stride;
    double v = (i == j) ? 1.0 : 0.0;
    if (i < n && j < n) {
        const double S0 = st[1], fact = 1.0 - st[2] / (S0 * S0);
        const double c = gm_cov_entry(st, n, i, j, S0, fact);
        if (cov_out) cov_out[(g * n + i) * n + j] = c;
        if (!bad[g]) v = c;
    }
    A[g * np * np + idx] = v;
}

// F[g][i][j] = (j >= i) ? L[g][j][i] : 0 for the groups that factored; flags: 1 bad moments, 2 not positive definite
__global__ void __launch_bounds__(GM_TB) k_gm_store(const double *L, int64_t n, int64_t np, const int32_t *bad,
                                                    const int32_t *notpsd, double *F, int32_t *flags)
{
    const int64_t g = blockIdx.y;
    const int flag = bad[g] ? 1 : (notpsd[g] ? 2 : 0);
    const int64_t idx = (int64_t)blockIdx.x * GM_TB + threadIdx.x;
    if (idx == 0) flags[g] = flag;
    if (flag || idx >= n * n) return;
    const int64_t i = idx / n, j = idx - i * n;
    F[g * n * n + idx] = (j >= i) ? L[(g * np + j) * np + i] : 0.0;
}

int launch_group_moments_factor(beatamd_ctx *ctx, int64_t G, int64_t n, const double *state, double *factor, double *cov,
                                int32_t *flags)
{
    const int64_t stride = group_moments_stride(n);
    const int64_t np = (n + 63) / 64 * 64;
    double *A;
    int32_t *bad;
    BA_TRY(ctx->scratch(SL_CHOL_A, (size_t)G * np * np, &A));
    BA_TRY(ctx->scratch(SL_GM_FLAG, (size_t)2 * G, &bad));
    int32_t *notpsd = bad + G;
    ScopedTimer tm(ctx, "group_factor");
    hipLaunchKernelGGL(k_gm_check, dim3((unsigned)G), dim3(GM_TB), 0, ctx->stream, state, stride, n, bad);
    hipLaunchKernelGGL(k_gm_cov, dim3((unsigned)((np * np + GM_TB - 1) / GM_TB), (unsigned)G), dim3(GM_TB), 0, ctx->stream,
                       state, stride, n, np, (const int32_t *)bad, A, cov);
    BA_TRY(launch_potrf_lower(ctx, G, np, A, notpsd));
    hipLaunchKernelGGL(k_gm_store, dim3((unsigned)((n * n + GM_TB - 1) / GM_TB), (unsigned)G), dim3(GM_TB), 0, ctx->stream,
                       (const double *)A, n, np, (const int32_t *)bad, (const int32_t *)notpsd, factor, flags);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
