// resolution.hip -- the dense FP64 pieces of the resolution-based fault discretization (Atzori & Antonioli 2011,
// Atzori et al. 2019; reference beat/ffi/fault.py:1520-1987 optimize_discretization) that had no kernel:
//
//   k_smooth_corr_fill / k_smooth_corr_diag   get_smoothing_operator_correlated (beat/models/laplacian.py:261-298)
//   launch_model_resolution                   R = inv(Gd^T Gd) . G^T G, Gd = vstack(G, eps^2 L)  (fault.py:1802-1816)
//   k_patch_data_min / k_division_rating      the division penalties and their product (fault.py:1884-1934)
//
// Contraction is off in this file (Makefile): every sum below is a chain of separately rounded additions in the
// stated order, so the host restatements (beat_amd/models/laplacian.py, tests/discretization_ref.py) give the same bits
// wherever sqrt, the division and exp round as numpy's do.
#include "kernels.hpp"

namespace beatamd {

// ------------------------------------------------------------------ correlated smoothing operator
// utility.distances (utility.py:1695-1723): sqrt(power(p - r, 2).sum(axis=2)): the three squares are summed in axis
// order, ((dx^2 + dy^2) + dz^2).
__device__ __forceinline__ double dist3(const double *c, int64_t i, int64_t j)
{
    const double dx = c[i * 3 + 0] - c[j * 3 + 0], dy = c[i * 3 + 1] - c[j * 3 + 1], dz = c[i * 3 + 2] - c[j * 3 + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// a[i][j] = 1 / d^2 ("gaussian", kind 0) or 1 / exp(d) ("exponential", kind 1), zero on the diagonal
// (laplacian.py:279-295: the diagonal distance is set to one first and the entry to zero afterwards)
__global__ void __launch_bounds__(256) k_smooth_corr_fill(const double *coords, int64_t P, int kind, double *a)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= P * P) return;
    const int64_t i = idx / P, j = idx - i * P;
    double v = 0.0;
    if (i != j) {
        const double d = dist3(coords, i, j);
        v = kind == 0 ? 1.0 / (d * d) : 1.0 / exp(d);
    }
    a[idx] = v;
}

// norm_distances = a.sum(0); fill_diagonal(a, -norm_distances) (laplacian.py:296-297).  One thread per column, the
// rows added in ascending order from zero: the order numpy's a.sum(0) takes on a C-contiguous array at every P
// (its pairwise blocks serve reductions along the contiguous axis only).
__global__ void __launch_bounds__(256) k_smooth_corr_diag(int64_t P, double *a)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= P) return;
    double s = 0.0;
    for (int64_t i = 0; i < P; i++) s += a[i * P + j];   // (the diagonal entry is zero here)
    a[j * P + j] = -s;
}

int launch_smoothing_correlated(beatamd_ctx *ctx, int64_t P, const double *coords, int kind, double *L)
{
    if (P == 0) return BEATAMD_OK;
    BA_CHECK(P * P < ((int64_t)1 << 38), BEATAMD_EINVAL, "smoothing_correlated: too many patches");
    ScopedTimer tm(ctx, "smooth_corr");
    hipLaunchKernelGGL(k_smooth_corr_fill, dim3((unsigned)((P * P + 255) / 256)), dim3(256), 0, ctx->stream, coords, P,
                       kind, L);
    hipLaunchKernelGGL(k_smooth_corr_diag, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, ctx->stream, P, L);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ------------------------------------------------------------------ model resolution matrix
// T[j][i] = s * S[i][j] for a square matrix (16 x 16 tiles through LDS)
__global__ void __launch_bounds__(256) k_res_transpose(const double *S, int64_t n, double s, double *T)
{
    __shared__ double tile[16][17];
    const int64_t i0 = (int64_t)blockIdx.x * 16, j0 = (int64_t)blockIdx.y * 16;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    if (i0 + ty < n && j0 + tx < n) tile[ty][tx] = S[(i0 + ty) * n + j0 + tx];
    __syncthreads();
    if (j0 + ty < n && i0 + tx < n) T[(j0 + ty) * n + i0 + tx] = s * tile[tx][ty];
}

__global__ void __launch_bounds__(256) k_res_diag(const double *R, int64_t n, double *diag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) diag[i] = R[i * n + i];
}

// gfs [P, nobs] are the library rows, i.e. G^T of the reference's G(nobs, npatches) (fault.py:1738); L [P, P].
// The reference inverts the normal matrix N = G^T G + eps^4 L^T L with LAPACK's LU.  N is symmetric positive
// definite wherever that inverse means anything, so the factor is Cholesky's: launch_chol_inverse (the blocked
// potrf_lower + the blocked triangular inverse chol.hip already has) gives the upper-triangular W with
// inv(N) = W^T W, and R comes from the factor's inverse with two matrix-core products on the transposed side,
//     R^T = G^T G . inv(N) = (G^T G . W^T) . W      (G^T G and N symmetric),
// then one transposition.  A blocked triangular solve with P right-hand sides would save a third of the flops of
// this step and cost a new kernel; at the P of a discretization (tens to a few thousand) the factor dominates
// neither way.  A matrix that is not positive definite raises the status word -> BEATAMD_ENOTPSD.
int launch_model_resolution(beatamd_ctx *ctx, int64_t P, int64_t nobs, const double *gfs, const double *L,
                            double epsilon, double *R, double *diag)
{
    if (P == 0) return BEATAMD_OK;
    BA_CHECK(gfs && L && R && diag && nobs > 0 && P <= 32768, BEATAMD_EINVAL, "model_resolution: bad argument");
    double *GG, *N, *W, *T, *U, *logd;
    const size_t pp = (size_t)P * P;
    BA_TRY(ctx->scratch(SL_RES_GG, pp, &GG));
    BA_TRY(ctx->scratch(SL_RES_N, pp, &N));
    BA_TRY(ctx->scratch(SL_RES_W, pp, &W));
    BA_TRY(ctx->scratch(SL_RES_T, pp, &T));
    BA_TRY(ctx->scratch(SL_RES_U, pp + 1, &U));
    logd = U + pp;
    ScopedTimer tm(ctx, "model_resolution");
    const dim3 tgrid((unsigned)((P + 15) / 16), (unsigned)((P + 15) / 16));
    GemmCall g;   // GG = gfs . gfs^T = G^T G
    g.A = gfs; g.lda = nobs; g.B = gfs; g.ldb = nobs; g.O = GG; g.ldo = P;
    g.M = P; g.N = P; g.K = nobs; g.b_kn = 0; g.timer = "resolution_gemm";
    BA_TRY(launch_gemm_f64(ctx, g));
    // N = GG + (eps^2 L)^T (eps^2 L): the smoothing operator is scaled first, as fault.py:1805-1808 does
    hipLaunchKernelGGL(k_res_transpose, tgrid, dim3(256), 0, ctx->stream, L, P, epsilon * epsilon, U);
    BA_HIP(hipMemcpyAsync(N, GG, pp * 8, hipMemcpyDeviceToDevice, ctx->stream));
    GemmCall h;
    h.A = U; h.lda = P; h.B = U; h.ldb = P; h.O = N; h.ldo = P;
    h.M = P; h.N = P; h.K = P; h.b_kn = 0; h.accumulate = 1; h.timer = "resolution_gemm";
    BA_TRY(launch_gemm_f64(ctx, h));
    BA_TRY(launch_chol_inverse(ctx, 1, P, N, W, logd));
    GemmCall p;   // T = GG . W^T
    p.A = GG; p.lda = P; p.B = W; p.ldb = P; p.O = T; p.ldo = P;
    p.M = P; p.N = P; p.K = P; p.b_kn = 0; p.b_upper = 1; p.timer = "resolution_gemm";
    BA_TRY(launch_gemm_f64(ctx, p));
    GemmCall q;   // U = T . W = R^T
    q.A = T; q.lda = P; q.B = W; q.ldb = P; q.O = U; q.ldo = P;
    q.M = P; q.N = P; q.K = P; q.b_kn = 1; q.timer = "resolution_gemm";
    BA_TRY(launch_gemm_f64(ctx, q));
    hipLaunchKernelGGL(k_res_transpose, tgrid, dim3(256), 0, ctx->stream, (const double *)U, P, 1.0, R);
    hipLaunchKernelGGL(k_res_diag, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)R, P,
                       diag);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ------------------------------------------------------------------ division rating
// horizontal distance of two points given as (east, north) pairs: distances() on two columns
__device__ __forceinline__ double dist2(double ax, double ay, double bx, double by)
{
    const double dx = ax - bx, dy = ay - by;
    return sqrt(dx * dx + dy * dy);
}

// dmin[j] = min over the observation points of the horizontal distance to the centre of patch j
// (fault.py:1915-1918: distances(data_coords, centers).min(axis=0)).  One workgroup per patch; min is order-free.
__global__ void __launch_bounds__(256) k_patch_data_min(int64_t P, int64_t nobs, const double *centers,
                                                        const double *data_en, double *dmin)
{
    __shared__ double red[256];
    const int64_t j = blockIdx.x;
    const double cx = centers[j * 3 + 0], cy = centers[j * 3 + 1];
    double m = INFINITY;
    for (int64_t k = threadIdx.x; k < nobs; k += 256) m = fmin(m, dist2(data_en[k * 2], data_en[k * 2 + 1], cx, cy));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) dmin[j] = red[0];
}

// rating[i] = area * c1 * c2 * c3 (fault.py:1929, multiplied from the left), one thread per patch:
//   area = width * length                                                      :1893
//   c1   = exp(((-depth_penalty * center_z) * km) / bottom_depth)              :1903-1907, left to right
//   c2   = min_j(dmin) / dmin[i]                                               :1920
//   c3   = (sum_j mean_R[j] * d[i][j]) / (sum_i' d[i'][i])                     :1925-1927
// with d the horizontal distances between the patch centres.  Both sums of c3 run over the other index in ascending
// order from zero (numpy's res_w.sum(axis=1) is pairwise instead, its sum(0) is this order: restated in
// tests/discretization_ref.py; the two differ by rounding only).
__global__ void __launch_bounds__(256) k_division_rating(int64_t P, const double *widths, const double *lengths,
                                                         const double *centers, const double *bottom_depth,
                                                         double depth_penalty, const double *dmin,
                                                         const double *mean_R, double *rating)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const double cx = centers[i * 3 + 0], cy = centers[i * 3 + 1], cz = centers[i * 3 + 2];
    double gmin = INFINITY, num = 0.0, den = 0.0;
    for (int64_t j = 0; j < P; j++) {
        gmin = fmin(gmin, dmin[j]);
        const double ox = centers[j * 3 + 0], oy = centers[j * 3 + 1];
        num += mean_R[j] * dist2(cx, cy, ox, oy);     // res_w[i][j] = mean_R[j] * d[i][j]
        den += dist2(ox, oy, cx, cy);                 // d[j][i]
    }
    const double area = widths[i] * lengths[i];
    const double c1 = exp(((-depth_penalty * cz) * 1000.0) / bottom_depth[i]);
    const double c2 = gmin / dmin[i];
    const double c3 = num / den;
    rating[i] = ((area * c1) * c2) * c3;
}

int launch_division_rating(beatamd_ctx *ctx, int64_t P, int64_t nobs, const double *widths, const double *lengths,
                           const double *centers, const double *bottom_depth, double depth_penalty,
                           const double *data_en, const double *mean_R, double *dmin, double *rating)
{
    if (P == 0) return BEATAMD_OK;
    BA_CHECK(nobs > 0 && P < (int64_t)0x7fffffff, BEATAMD_EINVAL, "division_rating: bad argument");
    ScopedTimer tm(ctx, "division_rating");
    hipLaunchKernelGGL(k_patch_data_min, dim3((unsigned)P), dim3(256), 0, ctx->stream, P, nobs, centers, data_en, dmin);
    hipLaunchKernelGGL(k_division_rating, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, ctx->stream, P, widths,
                       lengths, centers, bottom_depth, depth_penalty, (const double *)dmin, mean_R, rating);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
