// smc.hip -- the sampler steps around the forward model, on the device: SMC stage transition
// (tempering step, importance weights, systematic resampling, proposal factor), row gathers for the
// population / replica exchange, and the Metropolis step: proposal rows from an own counter-based
// generator, propose, accept, per-chain step-size tuning (its rules: philox.hpp, metropolis.hpp).
// The population never leaves HBM between stages; only the new beta (and acceptance counts) go
// back to the host.
//
// Reference arithmetic (hvasbath/beat):
//   SMC.calc_beta        beat/sampler/smc.py:133-165   bisection on the coefficient of variation
//   SMC.calc_covariance  beat/sampler/smc.py:167-186   np.cov(population, aweights=weights)
//   SMC.resample         beat/sampler/smc.py:290-324   Kitagawa's deterministic resampling
//   proposal draws       beat/sampler/base.py:35-71, 163-186; metropolis.py:289-292
//   step-size tuning     beat/sampler/metropolis.py:294-306 (pymc's tune table)
//
// All reductions run in a fixed order that does not depend on the launch (one workgroup, fixed
// width), so every rank of a multi-GPU run computes bit-identical stage decisions from the same
// gathered arrays.
#include "kernels.hpp"
#include "metropolis.hpp"
#include "wave.hpp"

namespace beatamd {

constexpr int SMC_TB = 1024;  // one workgroup of 16 wavefronts

// smc.py:133-165.  mode 0: bisection -> out[0] = new beta, out[1] = old beta, weights of the last
// bisection midpoint (exactly what the reference returns: `temp` of the final loop iteration).
// mode 1: weights for a given exponent step dbeta (final stage, smc.py:526-529).
__global__ void __launch_bounds__(SMC_TB) k_smc_calc_beta(const double *lik, int64_t stride, int64_t n,
                                                         double beta, double cv, int mode,
                                                         double dbeta, double *out, double *weights)
{
    __shared__ double sh[SMC_TB / 64];
    const int tid = threadIdx.x;
    double m = -INFINITY;
    for (int64_t i = tid; i < n; i += SMC_TB) m = fmax(m, lik[i * stride]);
    const double lmax = block_max_waveorder(m, sh);

    double low = beta, up = 2.0, cur = beta, total = 0.0;
    double step = dbeta;
    bool more = (mode == 1) || (up - low > 1e-6);
    while (more) {
        if (mode == 0) {
            cur = (low + up) / 2.0;
            step = cur - beta;
        }
        double s = 0.0;
        for (int64_t i = tid; i < n; i += SMC_TB) s += exp(step * (lik[i * stride] - lmax));
        total = block_sum_waveorder(s, sh);
        if (mode == 1) break;
        const double mean = total / (double)n;
        double q = 0.0;
        for (int64_t i = tid; i < n; i += SMC_TB) {
            const double d = exp(step * (lik[i * stride] - lmax)) - mean;
            q += d * d;
        }
        const double var = block_sum_waveorder(q, sh) / (double)n;
        const double cov_temp = sqrt(var) / mean;     // np.std(temp) / np.mean(temp)
        if (cov_temp > cv) up = cur; else low = cur;
        more = up - low > 1e-6;
    }
    for (int64_t i = tid; i < n; i += SMC_TB)
        weights[i] = exp(step * (lik[i * stride] - lmax)) / total;
    if (tid == 0) {
        out[0] = cur;
        out[1] = beta;
    }
}

int launch_smc_calc_beta(beatamd_ctx *ctx, int64_t n, const double *lik, int64_t stride, double beta,
                         double cv, int mode, double dbeta, double *out2, double *weights)
{
    ScopedTimer tm(ctx, "stage");
    hipLaunchKernelGGL(k_smc_calc_beta, dim3(1), dim3(SMC_TB), 0, ctx->stream, lik, stride, n, beta,
                       cv, mode, dbeta, out2, weights);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// smc.py:290-324.  cum_dist = np.cumsum(weights) is a sequential sum: one lane reproduces it
// term by term (bit-exact; 4096 chains ~ 20 us); the children are then placed by binary search:
// the reference's running index j is the smallest j with u[i] <= cum_dist[j], capped at n-1
// (SURVEY A.15 overrun guard), and np.repeat(parents, N_childs) lists exactly those j in order.
__global__ void __launch_bounds__(SMC_TB) k_smc_resample(const double *weights, int64_t n, double aux,
                                                        double *cum, int32_t *idx)
{
    if (threadIdx.x == 0) {
        double c = 0.0;
        int64_t i = 0;
        for (; i + 8 <= n; i += 8) {
            double w[8];
#pragma unroll
            for (int e = 0; e < 8; e++) w[e] = weights[i + e];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                c += w[e];
                cum[i + e] = c;
            }
        }
        for (; i < n; i++) {
            c += weights[i];
            cum[i] = c;
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int64_t i = threadIdx.x; i < n; i += SMC_TB) {
        const double u = ((double)i + aux) / (double)n;
        int64_t lo = 0, hi = n - 1;          // answer in [0, n-1]
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (u > cum[mid]) lo = mid + 1; else hi = mid;
        }
        idx[i] = (int32_t)lo;
    }
}

int launch_smc_resample(beatamd_ctx *ctx, int64_t n, const double *weights, double aux, double *cum,
                        int32_t *idx)
{
    ScopedTimer tm(ctx, "stage");
    hipLaunchKernelGGL(k_smc_resample, dim3(1), dim3(SMC_TB), 0, ctx->stream, weights, n, aux, cum, idx);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// Proposal factor of the weighted population (smc.py:167-186 np.cov(X, aweights=w, bias=False)):
// with v1 = sum w, v2 = sum w^2, mean_j = sum_i w_i x_ij / v1 and
//     F[i, j] = sqrt(w_i / (v1 - v2 / v1)) * (x_ij - mean_j)
// F^T F is that covariance, so rows z . F (z standard normal) are N(0, cov) draws without
// forming or factoring an (often singular) nparams x nparams matrix.  One workgroup per 64
// parameter columns: 64 columns x 4 row groups, fixed-order sums.
__global__ void __launch_bounds__(256) k_pop_factor(const double *X, int64_t ldx, const double *w,
                                                   int64_t n, int64_t np, double *F, int *status)
{
    __shared__ double sh[4][64];
    __shared__ double shw[8];
    const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;
    const int64_t j = (int64_t)blockIdx.x * 64 + col;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t i = tid; i < n; i += 256) {
        const double wi = w[i];
        s1 += wi;
        s2 += wi * wi;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {   // two wave_butterfly<OpAdd> (wave.hpp) in one loop: open-coded
        s1 += __shfl_xor(s1, off, 64);
        s2 += __shfl_xor(s2, off, 64);
    }
    if (col == 0) { shw[rg] = s1; shw[4 + rg] = s2; }
    __syncthreads();
    const double v1 = ((shw[0] + shw[1]) + shw[2]) + shw[3];
    const double v2 = ((shw[4] + shw[5]) + shw[6]) + shw[7];
    double m = 0.0;
    if (j < np)
        for (int64_t i = rg; i < n; i += 4) m = fma(w[i], X[i * ldx + j], m);
    sh[rg][col] = m;
    __syncthreads();
    const double mean = (((sh[0][col] + sh[1][col]) + sh[2][col]) + sh[3][col]) / v1;
    const double fact = 1.0 / (v1 - v2 / v1);
    // degenerate weights (one chain carries everything: v1 - v2/v1 = 0) or a non-finite population:
    // the reference's calc_covariance raises (smc.py:181-185); here the status word carries it to the
    // next synchronisation
    bool bad = !(v1 - v2 / v1 > 0.0);
    if (j < np)
        for (int64_t i = rg; i < n; i += 4) {
            const double f = sqrt(w[i] * fact) * (X[i * ldx + j] - mean);
            bad = bad || !isfinite(f);
            F[i * np + j] = f;
        }
    if (__any(bad) && (tid & 63) == 0) atomicOr(status, ST_BAD_COV);
}

int launch_pop_factor(beatamd_ctx *ctx, int64_t n, int64_t np, const double *X, int64_t ldx,
                      const double *w, double *F)
{
    if (n == 0 || np == 0) return BEATAMD_OK;
    ScopedTimer tm(ctx, "stage");
    hipLaunchKernelGGL(k_pop_factor, dim3((unsigned)((np + 63) / 64)), dim3(256), 0, ctx->stream, X,
                       ldx, w, n, np, F, ctx->d_status);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// out[i, :] = src[idx[i], :]   (resampled parents -> chain starts, smc.py:188-240 / base.py:541-571;
// replica exchange permutation, pt.py:573-633)
__global__ void __launch_bounds__(256) k_gather_rows(const double *src, int64_t lds, const int32_t *idx,
                                                    int64_t nrow_src, int64_t ncol, double *out,
                                                    int64_t ldo, int *status)
{
    const int64_t r = blockIdx.x;
    int64_t s = idx[r];
    if (s < 0 || s >= nrow_src) {
        if (threadIdx.x == 0) atomicOr(status, ST_INDEX_OOB);
        s = 0;
    }
    for (int64_t k = threadIdx.x; k < ncol; k += 256) out[r * ldo + k] = src[s * lds + k];
}

int launch_gather_rows(beatamd_ctx *ctx, int64_t nout, int64_t ncol, const double *src, int64_t lds,
                       int64_t nrow_src, const int32_t *idx, double *out, int64_t ldo)
{
    if (nout == 0 || ncol == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)nout), dim3(256), 0, ctx->stream, src, lds, idx,
                       nrow_src, ncol, out, ldo, ctx->d_status);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// metropolis.py:294-306 with pymc's tune table (tune_factor, metropolis.hpp)
__global__ void __launch_bounds__(256) k_tune_scaling(int64_t C, double *scaling, int32_t *accepted,
                                                     double interval)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double f = tune_factor((double)accepted[c] / interval);
    scaling[c] = scaling[c] * f;
    accepted[c] = 0;
}

int launch_tune_scaling(beatamd_ctx *ctx, int64_t C, double *scaling, int32_t *accepted, double interval)
{
    if (C == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_tune_scaling, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, ctx->stream, C,
                       scaling, accepted, interval);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// accepted_total[c] += accepted[c]  (per-stage acceptance bookkeeping stays on the device)
__global__ void __launch_bounds__(256) k_accumulate_i32(int64_t C, const int32_t *a, int32_t *acc)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < C) acc[c] += a[c];
}

int launch_accumulate_i32(beatamd_ctx *ctx, int64_t C, const int32_t *a, int32_t *acc)
{
    if (C == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_accumulate_i32, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, ctx->stream,
                       C, a, acc);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 draws (generator, counter layout, streams and every transform: philox.hpp)
//   stream 0: proposal normals z[c, 2j], z[c, 2j+1] from pair j of chain c
__global__ void __launch_bounds__(256) k_philox_normal(double *z, int64_t C, int64_t K, uint64_t seed,
                                                      uint32_t step, uint64_t first_chain, const uint32_t *step_dev)
{
    if (step_dev) step = *step_dev;   // device-resident step counter (graph replay): replaces the argument
    const int64_t npair = (K + 1) / 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C * npair) return;
    const int64_t c = i / npair, j = i - c * npair;
    const uint64_t gc = first_chain + (uint64_t)c;
    uint32_t r[4];
    philox4x32_10((uint32_t)j, (uint32_t)gc, step, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    double a, b;
    box_muller(r, a, b);
    z[c * K + 2 * j] = a;
    if (2 * j + 1 < K) z[c * K + 2 * j + 1] = b;
}

// per chain: log of the Metropolis uniform (metrop_select) and, for a multivariate-t proposal with
// df degrees of freedom, the row scale 1 / sqrt(chi2(df) / df)  (base.py:63-71)
__global__ void __launch_bounds__(256) k_philox_chain(int64_t C, uint64_t seed, uint32_t step,
                                                     uint64_t first_chain, int df, double *log_u,
                                                     double *row_scale, const uint32_t *step_dev)
{
    if (step_dev) step = *step_dev;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const uint32_t gc = (uint32_t)(first_chain + (uint64_t)c), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (log_u) log_u[c] = philox_log_u(gc, step, k0, k1);
    if (row_scale) row_scale[c] = philox_t_row_scale(gc, step, df, k0, k1);
}

// per-parameter proposal families (reference beat/sampler/base.py:129-160; kinds 0..3: philox_scaled_pair): every
// component of a row is an independent draw times the parameter's scale.  One thread per (chain, pair of parameters).
__global__ void __launch_bounds__(256) k_philox_univariate(double *delta, int64_t C, int64_t np, int kind,
                                                          const double *scale, uint64_t seed, uint32_t step,
                                                          uint64_t first_chain, const uint32_t *step_dev, int *status)
{
    if (step_dev) step = *step_dev;
    const int64_t npair = (np + 1) / 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C * npair) return;
    const int64_t c = i / npair, j = i - c * npair;
    const uint64_t gc = first_chain + (uint64_t)c;
    const bool second = 2 * j + 1 < np;   // (a row of odd length has no second component in its last pair)
    double a, b;
    philox_scaled_pair(kind, (uint32_t)j, (uint32_t)gc, step, (uint32_t)seed, (uint32_t)(seed >> 32), scale[2 * j],
                       second ? scale[2 * j + 1] : 0.0, status, a, b);
    delta[c * np + 2 * j] = a;
    if (second) delta[c * np + 2 * j + 1] = b;
}

int launch_philox_univariate(beatamd_ctx *ctx, double *delta, int64_t C, int64_t np, int kind,
                             const double *scale, uint64_t seed, uint32_t step, uint64_t first_chain)
{
    const int64_t n = C * ((np + 1) / 2);
    if (n == 0) return BEATAMD_OK;
    ScopedTimer tm(ctx, "proposal");
    hipLaunchKernelGGL(k_philox_univariate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       delta, C, np, kind, scale, seed, step, first_chain, ctx->step_dev, ctx->d_status);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_philox_normal(beatamd_ctx *ctx, double *z, int64_t C, int64_t K, uint64_t seed,
                         uint32_t step, uint64_t first_chain)
{
    const int64_t n = C * ((K + 1) / 2);
    if (n == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_philox_normal, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, z,
                       C, K, seed, step, first_chain, ctx->step_dev);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_philox_chain(beatamd_ctx *ctx, int64_t C, uint64_t seed, uint32_t step, uint64_t first_chain,
                        int df, double *log_u, double *row_scale)
{
    if (C == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_philox_chain, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, ctx->stream, C,
                       seed, step, first_chain, df, log_u, row_scale, ctx->step_dev);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ---- small parameter vectors (geometry mode: ~10 parameters, ~1000 chains): the whole proposal of a
// step in ONE launch -- the draws of k_philox_normal / k_philox_chain / k_philox_univariate (the same
// philox.hpp functions on the same counters, so the same numbers), the factor product of the proposal GEMM
// (k ascending, one FMA chain per component: the one piece k_draw_propose states itself) and k_propose's
// propose_component with a chain parked on q0 outside the box.  A workgroup serves DP_CB chains; factor,
// normals and flags sit in LDS.
constexpr int DP_CB = 16, DP_MAX = 64;

struct DrawProposeArgs {
    int64_t C, K, np;
    int kind;                 // -1 multivariate (factor [K, np], df), else the univariate family
    const double *factor;     // [K, np] or the per-parameter scales [np]
    int64_t cpg, sF;          // chains per proposal group (C: one factor for all) and the factors' stride
    int df;
    uint64_t seed, first_chain;
    uint32_t step;
    const uint32_t *step_dev;
    int *status;
    const double *Q0, *scaling, *lower, *upper;
    double *Qprop, *log_u;
    int32_t *inbounds;
};

__global__ void __launch_bounds__(256) k_draw_propose(DrawProposeArgs a)
{
    __shared__ double Fs[DP_MAX * DP_MAX];
    __shared__ double zs[DP_CB][DP_MAX];
    __shared__ double rs[DP_CB];
    __shared__ int ok[DP_CB];
    const uint32_t step = a.step_dev ? *a.step_dev : a.step;
    const int tid = threadIdx.x;
    // a workgroup's chains share a factor: the groups are cut into workgroups one by one
    const int64_t bpg = (a.cpg + DP_CB - 1) / DP_CB, grp = (int64_t)blockIdx.x / bpg;
    const int64_t c0 = grp * a.cpg + ((int64_t)blockIdx.x - grp * bpg) * DP_CB;
    const int nc = (int)min((int64_t)DP_CB, (grp + 1) * a.cpg - c0);
    const double *factor = a.factor + grp * a.sF;
    const int K = (int)a.K, np = (int)a.np;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    if (a.kind < 0)
        for (int i = tid; i < K * np; i += 256) Fs[i] = factor[i];
    const int npair = (K + 1) / 2;
    for (int i = tid; i < nc * npair; i += 256) {
        const int c = i / npair, j = i - c * npair;
        const uint32_t gc = (uint32_t)(a.first_chain + (uint64_t)(c0 + c));
        double x, y;
        if (a.kind < 0) {
            uint32_t r[4];
            philox4x32_10((uint32_t)j, gc, step, 0u, k0, k1, r);
            box_muller(r, x, y);
        } else {
            philox_scaled_pair(a.kind, (uint32_t)j, gc, step, k0, k1, factor[2 * j],
                               (2 * j + 1 < K) ? factor[2 * j + 1] : 0.0, a.status, x, y);
        }
        zs[c][2 * j] = x;
        if (2 * j + 1 < K) zs[c][2 * j + 1] = y;
    }
    if (tid < nc) {
        const uint32_t gc = (uint32_t)(a.first_chain + (uint64_t)(c0 + tid));
        a.log_u[c0 + tid] = philox_log_u(gc, step, k0, k1);
        rs[tid] = (a.kind < 0 && a.df > 0) ? philox_t_row_scale(gc, step, a.df, k0, k1) : 1.0;
        ok[tid] = 1;
    }
    __syncthreads();
    for (int i = tid; i < nc * np; i += 256) {
        const int c = i / np, n = i - c * np;
        double o;
        if (a.kind < 0) {
            double acc = 0.0;
            for (int k = 0; k < K; k++) acc = fma(zs[c][k], Fs[k * np + n], acc);
            o = (a.df > 0) ? acc * rs[c] : acc;
        } else {
            o = zs[c][n];
        }
        const int64_t g = (c0 + c) * a.np + n;
        double q;
        const bool inside = propose_component(a.Q0[g], o, a.scaling[c0 + c], a.lower[n], a.upper[n], q);
        a.Qprop[g] = q;
        if (!inside) ok[c] = 0;
    }
    __syncthreads();
    for (int i = tid; i < nc * np; i += 256) {
        const int c = i / np;
        if (!ok[c]) {
            const int64_t g = (c0 + c) * a.np + (i - c * np);
            a.Qprop[g] = a.Q0[g];
        }
    }
    if (tid < nc) a.inbounds[c0 + tid] = ok[tid];
}

bool draw_propose_applicable(int64_t K, int64_t np) { return K >= 1 && K <= DP_MAX && np >= 1 && np <= DP_MAX; }

int launch_draw_propose(beatamd_ctx *ctx, int64_t C, int64_t K, int64_t np, int kind, const double *factor,
                        int df, uint64_t seed, uint32_t step, uint64_t first_chain, const double *Q0,
                        const double *scaling, const double *lower, const double *upper, double *Qprop,
                        double *log_u, int32_t *inbounds, int64_t groups)
{
    if (C == 0) return BEATAMD_OK;
    DrawProposeArgs a;
    a.C = C; a.K = K; a.np = np; a.kind = kind; a.factor = factor; a.df = df;
    a.cpg = C / groups; a.sF = groups > 1 ? K * np : 0;
    a.seed = seed; a.first_chain = first_chain; a.step = step; a.step_dev = ctx->step_dev;
    a.status = ctx->d_status;
    a.Q0 = Q0; a.scaling = scaling; a.lower = lower; a.upper = upper;
    a.Qprop = Qprop; a.log_u = log_u; a.inbounds = inbounds;
    ScopedTimer tm(ctx, "proposal");
    hipLaunchKernelGGL(k_draw_propose, dim3((unsigned)(groups * ((a.cpg + DP_CB - 1) / DP_CB))), dim3(256), 0, ctx->stream, a);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ---- the step around the forward model: propose before it, accept behind it
// metropolis.py:313-343: propose_component for every parameter of a chain; one workgroup per chain
__global__ void __launch_bounds__(256) k_propose(int64_t C, int64_t nparams, const double *Q0,
                                                const double *delta, const double *scaling,
                                                const double *lower, const double *upper,
                                                double *Qprop, int32_t *inbounds)
{
    const int64_t c = blockIdx.x;
    __shared__ int s_ok;
    if (threadIdx.x == 0) s_ok = 1;
    __syncthreads();
    const double sc = scaling[c];
    int ok = 1;
    for (int64_t k = threadIdx.x; k < nparams; k += 256) {
        double q;
        const bool inside = propose_component(Q0[c * nparams + k], delta[c * nparams + k], sc, lower[k], upper[k], q);
        Qprop[c * nparams + k] = q;
        if (!inside) ok = 0;
    }
    if (!ok) s_ok = 0;
    __syncthreads();
    // metropolis.py:341-343,383-385: outside the prior box the forward model is NOT evaluated
    // and the chain stays.  The batch evaluates every chain, so park the rejected chain on its
    // current point (keeps durations/start times inside the library grid).
    if (!s_ok)
        for (int64_t k = threadIdx.x; k < nparams; k += 256)
            Qprop[c * nparams + k] = Q0[c * nparams + k];
    if (threadIdx.x == 0) inbounds[c] = s_ok;
}

int launch_propose(beatamd_ctx *ctx, int64_t C, int64_t nparams, const double *Q0,
                   const double *delta, const double *scaling, const double *lower,
                   const double *upper, double *Qprop, int32_t *inbounds)
{
    if (C == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_propose, dim3((unsigned)C), dim3(256), 0, ctx->stream, C, nparams, Q0,
                       delta, scaling, lower, upper, Qprop, inbounds);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// metropolis.py:344-385 + pymc metrop_select: accept iff in bounds and metropolis_accept.
// One workgroup per chain.  Optional tail work of the step, so that a step needs no further launch:
//   grp.n > 0   the `like` column of the proposal is summed here (like_serial, as k_like_sum) from an
//               LDS copy of the row
//   acc_sum     per-chain acceptance counter (+= flag), n_acc the population total (+= flags)
//   step_dev    the device-resident Philox step counter moves on (read only by the draw kernels, which
//               precede this launch in stream order)
__global__ void __launch_bounds__(256) k_accept(int64_t C, int64_t nparams, int64_t nllk,
                                               double *Q0, double *L0, const double *Qprop,
                                               double *Lprop, const int32_t *inbounds,
                                               const double *log_u, double beta,
                                               const double *betas, int32_t *accepted, LikeGroups grp,
                                               const int32_t *chain_bad, int32_t *acc_sum,
                                               unsigned long long *n_acc, uint32_t *step_dev)
{
    extern __shared__ __attribute__((aligned(16))) double s_l[];
    const int64_t c = blockIdx.x;
    // a proposal outside the box is rejected without a look at its likelihood row: the forward model may have skipped it
    // (ffi_logp_device's `active`), the row then holds whatever an earlier step left there
    if (!inbounds[c]) {
        if (threadIdx.x == 0) {
            accepted[c] = 0;
            if (step_dev && c == 0) *step_dev += 1u;
        }
        return;
    }
    double lp;
    if (grp.n > 0) {
        for (int64_t k = threadIdx.x; k < nllk - 1; k += 256) s_l[k] = Lprop[c * nllk + k];
        __syncthreads();
        if (threadIdx.x == 0) {
            const double total = like_serial(s_l, grp, chain_bad && chain_bad[c]);
            s_l[nllk - 1] = total;
            Lprop[c * nllk + nllk - 1] = total;
        }
        __syncthreads();
        lp = s_l[nllk - 1];
    } else {
        lp = Lprop[c * nllk + nllk - 1];
    }
    const double b = betas ? betas[c] : beta;  // per-replica beta for parallel tempering
    const bool acc = metropolis_accept(b, lp, L0[c * nllk + nllk - 1], log_u[c]);
    if (acc) {
        for (int64_t k = threadIdx.x; k < nparams; k += 256) Q0[c * nparams + k] = Qprop[c * nparams + k];
        __syncthreads();  // all lanes have read L0[like] before it is overwritten
        if (grp.n > 0) {
            for (int64_t k = threadIdx.x; k < nllk; k += 256) L0[c * nllk + k] = s_l[k];
        } else {
            for (int64_t k = threadIdx.x; k < nllk; k += 256) L0[c * nllk + k] = Lprop[c * nllk + k];
        }
    }
    if (threadIdx.x == 0) {
        accepted[c] = acc ? 1 : 0;
        if (acc_sum && acc) acc_sum[c] += 1;
        if (n_acc && acc) atomicAdd(n_acc, 1ull);
        if (step_dev && c == 0) *step_dev += 1u;
    }
}

int launch_accept(beatamd_ctx *ctx, int64_t C, int64_t nparams, int64_t nllk, double *Q0,
                  double *L0, const double *Qprop, double *Lprop, const int32_t *inbounds,
                  const double *log_u, double beta, const double *betas, int32_t *accepted,
                  const LikeGroups *grp, const int32_t *chain_bad, int32_t *acc_sum, int64_t *n_acc,
                  bool advance_step)
{
    if (C == 0) return BEATAMD_OK;
    LikeGroups g;
    if (grp) g = *grp;
    const size_t lds = grp ? (size_t)nllk * sizeof(double) : 0;
    BA_CHECK(lds <= 48 * 1024, BEATAMD_EINVAL, "accept: likelihood vector of %lld entries", (long long)nllk);
    ScopedTimer tm(ctx, "astep");
    hipLaunchKernelGGL(k_accept, dim3((unsigned)C), dim3(256), lds, ctx->stream, C, nparams, nllk,
                       Q0, L0, Qprop, Lprop, inbounds, log_u, beta, betas, accepted, g, chain_bad, acc_sum,
                       (unsigned long long *)n_acc, advance_step ? ctx->step_dev : nullptr);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

__global__ void k_step_advance(uint32_t *step_dev) { *step_dev += 1u; }

// after the draws of a step: the device-resident counter moves on (captured with the step in a graph)
int launch_step_advance(beatamd_ctx *ctx)
{
    if (!ctx->step_dev) return BEATAMD_OK;
    hipLaunchKernelGGL(k_step_advance, dim3(1), dim3(1), 0, ctx->stream, ctx->step_dev);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
