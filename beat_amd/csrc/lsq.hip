// lsq.hip -- non-negative least-squares slip of a batch of chains (DistributionOptimizer.lsq_solution,
// beat/models/problems.py:753-873, the `initialization: lsq` start of an FFI run).
//
// With the rupture kinematics of a chain fixed the synthetics are linear in the inverted slip variable v; the reference
// builds the design matrix A [(T N + Nobs + P) x P] patch by patch and hands it to scipy.optimize.nnls.  Here A never
// exists: the kernels form the normal equations
//
//     N_c = sum_wm sum_t R_{c,t} R_{c,t}^T + G_v G_v^T + h_c^4 L^T L        b_c = sum_wm sum_t R_{c,t} d_t + G_v (d_geo - corr_c)
//
// (R_{c,t} [P x N]: the library rows the chain's start times and durations select for target t -- the row itself for
// nearest neighbour, the four-corner blend of beat/ffi/base.py:663-709 for multilinear) and solve them under x >= 0.
//
//   k_lsq_gram    seismic part of N_c on the FP64 matrix cores (v_mfma_f64_16x16x4_f64, lane layout of gemm.hip).  One
//                 256-thread workgroup owns one (chain, 64 x 64 tile pair of the lower triangle) and walks (target, 16-sample
//                 chunk) in ascending order through a double-buffered LDS stage (pitch 17); the rows are gathered through
//                 the index tables of k_gf_tables.  A further wavemap continues the same accumulators (they start from
//                 the stored tile), so the order of summation is (wavemap, target, sample) whatever the batch.
//   k_lsq_rhs     sum_t R_{c,t} d_t: one wavefront per (chain, patch), lanes strided over the samples, targets ascending,
//                 one butterfly sum at the end.
//   k_lsq_finish  adds the chain-independent blocks (lower triangle) and mirrors the upper triangle; the geodetic part of b.
//   k_nnls        Lawson-Hanson active set on (N_c, b_c): one wavefront per chain, Cholesky factor of the passive set in a
//                 per-chain scratch in global memory, vectors in LDS.
//   k_lsq_scatter v <- x, uperp <- 0 in the output points.
// Every reduction has a fixed order that depends on the chain alone: a chain's (N_c, b_c, x_c) is bit for bit the same
// alone, in any batch and on any rank.
#include <cmath>

#include "kernels.hpp"
#include "wave.hpp"

namespace beatamd {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int LQ_TB = 64, LQ_KB = 16, LQ_PITCH = LQ_KB + 1;

struct LsqSeisArgs {
    const double *G;          // library of the inverted variable [T, P, D, S, N]
    const uint32_t *rowoff;   // [C, T, P, nrow] (k_gf_tables, one table per target)
    const double *fac;        // [C, T, P, 4] multilinear
    const double *data;       // [T, N]
    double *Nmat, *b;         // [C, P, P], [C, P]
    int64_t C, T, P, N;
    int accumulate;           // continue the stored sums (second and further wavemaps)
    int ntb;                  // 64-patch blocks per side
};

// one sample of the row of R_{c,t} whose table cell is (ro, fa): the library row, or
// ((f_cc x_cc + f_fc x_fc) + f_cf x_cf) + f_ff x_ff with plain products and sums (numpy's order over the corner axis)
template <int ML>
__device__ __forceinline__ double lsq_row_value(const double *G, const uint32_t *ro, const double *fa, int64_t N, int64_t n)
{
    if (!ML) return G[(int64_t)ro[0] * N + n];
    double v = fa[0] * G[(int64_t)ro[0] * N + n];
    v = v + fa[1] * G[(int64_t)ro[1] * N + n];
    v = v + fa[2] * G[(int64_t)ro[2] * N + n];
    v = v + fa[3] * G[(int64_t)ro[3] * N + n];
    return v;
}

template <int ML>
__global__ void __launch_bounds__(256) k_lsq_gram(LsqSeisArgs a)
{
    constexpr int NROW = ML ? 4 : 1, NJ = LQ_TB / 16;
    __shared__ double As[2][LQ_TB * LQ_PITCH];
    __shared__ double Bs[2][LQ_TB * LQ_PITCH];

    const int64_t npair = (int64_t)a.ntb * (a.ntb + 1) / 2;
    const int64_t c = blockIdx.x / npair;
    const int pair = (int)(blockIdx.x % npair);
    // pair -> (bi, bj), bj <= bi, row-major over the lower triangle
    int bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= pair) bi++;
    const int bj = pair - bi * (bi + 1) / 2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t P = a.P, N = a.N, T = a.T;

    // staging role: row lr of both patch blocks, 4 consecutive samples from lk
    const int lr = tid >> 2, lk = (tid & 3) * 4;
    const int64_t pa = (int64_t)bi * LQ_TB + lr, pb = (int64_t)bj * LQ_TB + lr;
    const bool a_ok = pa < P, b_ok = pb < P;
    const int64_t nch = (N + LQ_KB - 1) / LQ_KB, nstep = T * nch;

    v4f64 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t row = (int64_t)bi * LQ_TB + wave * 16 + (lane >> 4) + 4 * r;
            const int64_t col = (int64_t)bj * LQ_TB + j * 16 + (lane & 15);
            acc[j][r] = (a.accumulate && row < P && col < P) ? a.Nmat[(c * P + row) * P + col] : 0.0;
        }
    }

    double av[4], bv[4];
    auto load_tile = [&](int64_t step) {
        const int64_t t = step / nch, n0 = (step - t * nch) * LQ_KB + lk;
        const int64_t cell = (c * T + t) * P;
        const uint32_t *roa = a.rowoff + (cell + (a_ok ? pa : 0)) * NROW;
        const uint32_t *rob = a.rowoff + (cell + (b_ok ? pb : 0)) * NROW;
        const double *faa = ML ? a.fac + (cell + (a_ok ? pa : 0)) * 4 : nullptr;
        const double *fab = ML ? a.fac + (cell + (b_ok ? pb : 0)) * 4 : nullptr;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const bool in = n0 + e < N;
            av[e] = (a_ok && in) ? lsq_row_value<ML>(a.G, roa, faa, N, n0 + e) : 0.0;
            bv[e] = (b_ok && in) ? lsq_row_value<ML>(a.G, rob, fab, N, n0 + e) : 0.0;
        }
    };
    if (nstep > 0) load_tile(0);
    int buf = 0;
    for (int64_t step = 0; step < nstep; step++) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            As[buf][lr * LQ_PITCH + lk + e] = av[e];
            Bs[buf][lr * LQ_PITCH + lk + e] = bv[e];
        }
        __syncthreads();
        if (step + 1 < nstep) load_tile(step + 1);
#pragma unroll
        for (int kk = 0; kk < LQ_KB / 4; kk++) {
            const int kcol = kk * 4 + (lane >> 4);
            const double aop = As[buf][(wave * 16 + (lane & 15)) * LQ_PITCH + kcol];
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                const double bop = Bs[buf][(j * 16 + (lane & 15)) * LQ_PITCH + kcol];
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop, bop, acc[j], 0, 0, 0);
            }
        }
        buf ^= 1;
    }
    // reg r of lane l -> row (l>>4) + 4r, column l&15 of the wave's 16 x 16 block j
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int64_t row = (int64_t)bi * LQ_TB + wave * 16 + (lane >> 4) + 4 * r;
        if (row >= P) continue;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int64_t col = (int64_t)bj * LQ_TB + j * 16 + (lane & 15);
            if (col < P) a.Nmat[(c * P + row) * P + col] = acc[j][r];
        }
    }
}

template <int ML>
__global__ void __launch_bounds__(256) k_lsq_rhs(LsqSeisArgs a)
{
    constexpr int NROW = ML ? 4 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;   // (chain, patch)
    if (item >= a.C * a.P) return;
    const int64_t c = item / a.P, p = item - c * a.P;
    double s = 0.0;
    for (int64_t t = 0; t < a.T; t++) {
        const int64_t cell = (c * a.T + t) * a.P + p;
        const uint32_t *ro = a.rowoff + cell * NROW;
        const double *fa = ML ? a.fac + cell * 4 : nullptr;
        const double *d = a.data + t * a.N;
        for (int64_t n = lane; n < a.N; n += 64) s = fma(lsq_row_value<ML>(a.G, ro, fa, a.N, n), d[n], s);
    }
    s = wave_butterfly<OpAdd>(s);
    if (lane == 0) a.b[item] = a.accumulate ? a.b[item] + s : s;
}

int launch_lsq_seismic(beatamd_ctx *ctx, const SeisLib &lib, int interp, int64_t C, const uint32_t *rowoff, const double *fac,
                       const double *data, int accumulate, double *Nmat, double *b)
{
    if (C == 0 || lib.P == 0) return BEATAMD_OK;
    LsqSeisArgs a;
    a.G = lib.g; a.rowoff = rowoff; a.fac = fac; a.data = data; a.Nmat = Nmat; a.b = b;
    a.C = C; a.T = lib.T; a.P = lib.P; a.N = lib.N; a.accumulate = accumulate;
    a.ntb = (int)((lib.P + LQ_TB - 1) / LQ_TB);
    const int64_t nblocks = C * ((int64_t)a.ntb * (a.ntb + 1) / 2), nrhs = (C * lib.P + 3) / 4;
    BA_CHECK(nblocks < (int64_t)0x7fffffff && nrhs < (int64_t)0x7fffffff, BEATAMD_EINVAL, "lsq: batch too large");
    const bool ml = interp == BEATAMD_MULTILINEAR;
    {
        ScopedTimer tm(ctx, "lsq_gram");
        if (ml) hipLaunchKernelGGL(k_lsq_gram<1>, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL(k_lsq_gram<0>, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, a);
        BA_HIP(hipGetLastError());
    }
    {
        ScopedTimer tm(ctx, "lsq_rhs");
        if (ml) hipLaunchKernelGGL(k_lsq_rhs<1>, dim3((unsigned)nrhs), dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL(k_lsq_rhs<0>, dim3((unsigned)nrhs), dim3(256), 0, ctx->stream, a);
        BA_HIP(hipGetLastError());
    }
    return BEATAMD_OK;
}

// ------------------------------------------------------------------ chain-independent blocks, mirror, geodetic right-hand side
__global__ void __launch_bounds__(256) k_lsq_transpose(const double *A, double *At, int64_t n)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * n) return;
    const int64_t i = idx / n, j = idx - i * n;
    At[idx] = A[j * n + i];
}

int launch_lsq_transpose(beatamd_ctx *ctx, const double *A, double *At, int64_t n)
{
    if (n == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_lsq_transpose, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, ctx->stream, A, At, n);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

struct LsqFinishArgs {
    int64_t C, P, Nobs, nparams, h_off;
    double *Nmat, *b;
    const double *GG, *LtL;       // [P, P] lower triangles (GG nullable)
    const double *Ggeo, *dgeo;    // [P, Nobs], [Nobs] (nullable)
    const double *Q;
    GeoCorr corr;
    int has_seis;                 // 0: N and b hold nothing yet
};

// one wavefront per (chain, row i): N[i, j] = seismic + GG + h^4 LtL for j <= i, stored at (i, j) and (j, i);
// b[i] += sum_k G[i, k] (d[k] - corr_c[k]), lanes strided over k, one butterfly sum
__global__ void __launch_bounds__(256) k_lsq_finish(LsqFinishArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;
    if (item >= a.C * a.P) return;
    const int64_t c = item / a.P, i = item - c * a.P, P = a.P;
    const double *Qc = a.Q + c * a.nparams;
    const double h = Qc[a.h_off];
    const double h2 = h * h, h4 = h2 * h2;   // (L h^2)^T (L h^2), problems.py:845-848
    double *Nc = a.Nmat + c * P * P;
    for (int64_t j = lane; j <= i; j += 64) {
        double v = a.has_seis ? Nc[i * P + j] : 0.0;
        if (a.GG) v = v + a.GG[i * P + j];
        v = v + h4 * a.LtL[i * P + j];
        Nc[i * P + j] = v;
        Nc[j * P + i] = v;
    }
    double s = 0.0;
    if (a.Ggeo) {
        const double *g = a.Ggeo + i * a.Nobs;
        for (int64_t k = lane; k < a.Nobs; k += 64) {
            // apply_corrections(displacements, point, operation="-") (geodetic.py:411-427): no odw factor
            const double r = geo_corr_subtract<false>(a.corr, Qc, a.corr.pole + c * a.corr.pole_stride, k, a.dgeo[k]);
            s = fma(g[k], r, s);
        }
        s = wave_butterfly<OpAdd>(s);
    }
    if (lane == 0) a.b[item] = a.has_seis ? a.b[item] + s : s;
}

int launch_lsq_finish(beatamd_ctx *ctx, int64_t C, int64_t P, double *Nmat, double *b, int has_seis, const double *GG,
                      const double *LtL, const double *Ggeo, int64_t Nobs, const double *dgeo, GeoCorr corr, const double *Q,
                      int64_t nparams, int64_t h_off)
{
    if (C == 0 || P == 0) return BEATAMD_OK;
    LsqFinishArgs a;
    a.C = C; a.P = P; a.Nobs = Nobs; a.nparams = nparams; a.h_off = h_off;
    a.Nmat = Nmat; a.b = b; a.GG = GG; a.LtL = LtL; a.Ggeo = Ggeo; a.dgeo = dgeo; a.Q = Q; a.corr = corr;
    a.has_seis = has_seis;
    const int64_t nb = (C * P + 3) / 4;
    BA_CHECK(nb < (int64_t)0x7fffffff, BEATAMD_EINVAL, "lsq: batch too large");
    ScopedTimer tm(ctx, "lsq_finish");
    hipLaunchKernelGGL(k_lsq_finish, dim3((unsigned)nb), dim3(256), 0, ctx->stream, a);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ------------------------------------------------------------------ non-negative least squares
// Lawson & Hanson's active set (Solving Least Squares Problems, ch. 23) on the normal equations, the form scipy's nnls
// iterates on (Bro & de Jong 1997): min |A x - d| s.t. x >= 0 with N = A^T A, b = A^T d.
//   w = b - N x; while some j outside the passive set has w_j > tol: add the largest (first of equals); solve
//   N_PP s_P = b_P; while min s_P < 0: alpha = min x_i / (x_i - s_i) over s_i < 0, x = x (1 - alpha) + alpha s, variables
//   with x <= tol leave the set, solve again; x = s.
// tol = 10 n 2^-52 max|b|.  The passive set is kept in the order of entry with the factor U (upper, U^T U = N_PP) in the
// chain's scratch [n, n] and z = U^-T b_P in LDS: entering is one forward substitution (a new column of U), a removal
// factors the remaining set again, every solve is one back substitution.  `iters` counts the solves (at least one per
// entered variable); at maxiter the chain stops with status 1 and the x it has.  Status 2: N or b not finite, or a
// passive block that is not numerically positive definite (x = NaN).
struct NnlsArgs {
    int n, maxiter;
    const double *Nmat, *b;   // [C, n, n], [C, n] of the chains of this launch
    double *x, *U;            // [C, n], scratch [C, n, n]
    int32_t *iters, *status;
};

// variable j enters the factor as passive variable m; false: the block is not positive definite
__device__ __forceinline__ bool nnls_append(const double *Nc, double *U, int n, int j, int m, int *pidx, double *y, double *r,
                                            double *z, const double *bb, int lane)
{
    for (int i = lane; i < m; i += 64) r[i] = Nc[(int64_t)pidx[i] * n + j];
    __syncthreads();
    for (int k = 0; k < m; k++) {
        const double yk = r[k] / U[(int64_t)k * n + k];
        for (int i = k + 1 + lane; i < m; i += 64) r[i] = r[i] - U[(int64_t)k * n + i] * yk;
        if (lane == 0) {
            U[(int64_t)k * n + m] = yk;
            y[k] = yk;
        }
        __syncthreads();
    }
    double s2 = 0.0, sz = 0.0;
    for (int k = lane; k < m; k += 64) {
        s2 = fma(y[k], y[k], s2);
        sz = fma(y[k], z[k], sz);
    }
    s2 = wave_butterfly<OpAdd>(s2);
    sz = wave_butterfly<OpAdd>(sz);
    const double d2 = Nc[(int64_t)j * n + j] - s2;
    if (!(d2 > 0.0) || !isfinite(d2)) return false;
    const double d = sqrt(d2);
    __syncthreads();
    if (lane == 0) {
        U[(int64_t)m * n + m] = d;
        z[m] = (bb[j] - sz) / d;
        pidx[m] = j;
    }
    __syncthreads();
    return true;
}

__global__ void __launch_bounds__(64) k_nnls(NnlsArgs a)
{
    extern __shared__ double nnls_sh[];
    const int n = a.n, lane = threadIdx.x;
    const int64_t c = blockIdx.x;
    double *x = nnls_sh, *w = x + n, *z = w + n, *r = z + n, *bb = r + n, *sp = bb + n;
    int *pidx = (int *)(sp + n), *inP = pidx + n;
    const double *Nc = a.Nmat + c * n * n, *bc = a.b + c * n;
    double *U = a.U + c * n * n, *xo = a.x + c * n;

    int bad = 0;
    double bmax = 0.0;
    for (int64_t i = lane; i < (int64_t)n * n; i += 64) bad |= !isfinite(Nc[i]);
    for (int i = lane; i < n; i += 64) {
        const double v = bc[i];
        bad |= !isfinite(v);
        bb[i] = v; w[i] = v; x[i] = 0.0; inP[i] = 0;
        bmax = fmax(bmax, fabs(v));
    }
    bmax = wave_butterfly<OpFmax>(bmax);
    int status = __any(bad) ? 2 : 0, np = 0, iter = 0;
    const double tol = 10.0 * n * 2.220446049250313e-16 * bmax;
    __syncthreads();

    while (status == 0 && np < n) {
        // the largest w outside the passive set, the first of equals
        double best = -INFINITY;
        int bj = n;
        for (int j = lane; j < n; j += 64)
            if (!inP[j] && w[j] > best) { best = w[j]; bj = j; }
        for (int off = 32; off > 0; off >>= 1) {   // (value, index) pairs: open-coded, see wave.hpp
            const double ob = __shfl_xor(best, off, 64);
            const int oj = __shfl_xor(bj, off, 64);
            if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
        }
        if (bj >= n || !(best > tol)) break;
        // (w is free until it is formed again: the new column of the factor is built in it)
        if (!nnls_append(Nc, U, n, bj, np, pidx, w, r, z, bb, lane)) { status = 2; break; }
        if (lane == 0) inP[bj] = 1;
        np++;
        __syncthreads();
        for (;;) {
            if (iter >= a.maxiter) { status = 1; break; }
            iter++;
            // U s = z, rows from the last: s_k = (z_k - sum_{i>k} U[k,i] s_i) / U[k,k]
            for (int k = np - 1; k >= 0; k--) {
                double part = 0.0;
                for (int i = k + 1 + lane; i < np; i += 64) part = fma(U[(int64_t)k * n + i], sp[i], part);
                part = wave_butterfly<OpAdd>(part);
                if (lane == 0) sp[k] = (z[k] - part) / U[(int64_t)k * n + k];
                __syncthreads();
            }
            double smin = INFINITY, alpha = INFINITY;
            for (int k = lane; k < np; k += 64) {
                const double sk = sp[k];
                smin = fmin(smin, sk);
                if (sk < 0.0) {
                    const double xi = x[pidx[k]];
                    alpha = fmin(alpha, xi / (xi - sk));
                }
            }
            for (int off = 32; off > 0; off >>= 1) {   // two wave_butterfly<OpFmin> (wave.hpp) in one loop: open-coded
                smin = fmin(smin, __shfl_xor(smin, off, 64));
                alpha = fmin(alpha, __shfl_xor(alpha, off, 64));
            }
            if (!(smin < 0.0)) break;
            for (int k = lane; k < np; k += 64) {
                const int j = pidx[k];
                double xi = x[j] * (1.0 - alpha);
                xi = xi + alpha * sp[k];
                x[j] = xi;
                if (xi <= tol) inP[j] = 0;
            }
            __syncthreads();
            // the remaining set in its order of entry, factored again (sp is free until the next solve: it keeps the
            // old order while pidx is rewritten)
            int *ord = (int *)sp;
            for (int k = lane; k < np; k += 64) ord[k] = pidx[k];
            __syncthreads();
            const int np_old = np;
            np = 0;
            bool ok = true;
            for (int k = 0; k < np_old && ok; k++) {
                const int j = ord[k];
                if (!inP[j]) {
                    if (lane == 0) x[j] = 0.0;
                    continue;
                }
                ok = nnls_append(Nc, U, n, j, np, pidx, w, r, z, bb, lane);
                np++;
            }
            __syncthreads();
            if (!ok) { status = 2; break; }
            if (np == 0) break;
        }
        if (status != 0) break;
        // x = s on the passive set, w = b - N x through the rows of the passive variables (N is symmetric)
        for (int k = lane; k < np; k += 64) x[pidx[k]] = sp[k];
        __syncthreads();
        for (int j = lane; j < n; j += 64) {
            double v = bb[j];
            for (int k = 0; k < np; k++) {
                const int pk = pidx[k];
                v = v - Nc[(int64_t)pk * n + j] * x[pk];
            }
            w[j] = v;
        }
        __syncthreads();
    }
    for (int i = lane; i < n; i += 64) xo[i] = status == 2 ? NAN : x[i];
    if (lane == 0) {
        a.iters[c] = iter;
        a.status[c] = status;
    }
}

int launch_nnls(beatamd_ctx *ctx, int64_t C, int64_t n, const double *Nmat, const double *b, double *x, int32_t *iters,
                int32_t *status, int maxiter)
{
    if (C == 0) return BEATAMD_OK;
    BA_CHECK(n >= 1 && n <= NNLS_MAX_N, BEATAMD_EINVAL, "nnls: %lld unknowns, 1 .. %d supported", (long long)n, NNLS_MAX_N);
    // chains per launch: the factors of a launch stay within NNLS_SCRATCH_BYTES
    const int64_t per = n * n * (int64_t)sizeof(double);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(C, NNLS_SCRATCH_BYTES / per));
    double *U;
    BA_TRY(ctx->scratch(SL_LSQ_U, (size_t)(chunk * n * n), &U));
    const size_t lds = (size_t)n * (6 * sizeof(double) + 2 * sizeof(int));
    ScopedTimer tm(ctx, "nnls");
    for (int64_t c0 = 0; c0 < C; c0 += chunk) {
        const int64_t cc = std::min(chunk, C - c0);
        NnlsArgs a;
        a.n = (int)n; a.maxiter = maxiter > 0 ? maxiter : (int)(3 * n);
        a.Nmat = Nmat + c0 * n * n; a.b = b + c0 * n; a.x = x + c0 * n; a.U = U;
        a.iters = iters + c0; a.status = status + c0;
        hipLaunchKernelGGL(k_nnls, dim3((unsigned)cc), dim3(64), lds, ctx->stream, a);
        BA_HIP(hipGetLastError());
    }
    return BEATAMD_OK;
}

// ------------------------------------------------------------------ the solution into the points
__global__ void __launch_bounds__(256) k_lsq_scatter(int64_t C, int64_t P, const double *x, double *Qout, int64_t nparams,
                                                     int64_t v_off, int64_t zero_off)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= C * P) return;
    const int64_t c = idx / P, p = idx - c * P;
    Qout[c * nparams + v_off + p] = x[idx];
    if (zero_off >= 0) Qout[c * nparams + zero_off + p] = 0.0;
}

int launch_lsq_scatter(beatamd_ctx *ctx, int64_t C, int64_t P, const double *x, double *Qout, int64_t nparams, int64_t v_off,
                       int64_t zero_off)
{
    if (C == 0 || P == 0) return BEATAMD_OK;
    hipLaunchKernelGGL(k_lsq_scatter, dim3((unsigned)((C * P + 255) / 256)), dim3(256), 0, ctx->stream, C, P, x, Qout, nparams,
                       v_off, zero_off);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
