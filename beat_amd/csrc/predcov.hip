// predcov.hip -- the velocity-model prediction covariance of the geodetic datasets (geodetic.py:1130-1202
// GeodeticDistributerComposite.update_weights): the synthetics of every crust variant at one point, their sample
// covariance per dataset, added to the dataset's resident data + pred_g covariance.  The factorisation that follows is
// chol.hip's; what is here is the arithmetic the reference does in numpy in front of it.
#include "kernels.hpp"

namespace beatamd {

// geodetic.py:1167-1176 / ffi/base.py:292-305: X[k, j] = sum_v sum_p G_{k,v}[p, j] * slip_v[p] for the K library variants
// of an ensemble at ONE point.  k_geo_stack with the variant axis where it has the chain axis: lane <-> observation
// column, variant <-> blockIdx.y, the nvar * P slips staged in LDS once per block.  Per (variant, column) exactly
// k_geo_stack's operation sequence -- variables ascending, patches ascending, one fma per term, the accumulator starting
// at 0 -- so the row of the variant that is the model's own library is bit for bit the mu of the likelihood.  A stream
// of K * nvar * P * Nobs * 8 bytes read once; two groups of sixteen loads in flight per lane as in k_geo_stack.  The
// library pointers come from a device table [K * nvar], variant-major.
struct CrustStackArgs {
    const double *const *G;   // device [K * nvar]
    const double *slips;      // device [nvar * P]
    int nvar;
    int64_t P, Nobs;
    double *X;                // [K, Nobs]
};

__global__ void __launch_bounds__(128) k_crust_stack(CrustStackArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_slip[];
    const int64_t P = a.P, Nobs = a.Nobs;
    const int64_t var = blockIdx.y;
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = threadIdx.x; i < a.nvar * P; i += blockDim.x) s_slip[i] = a.slips[i];
    __syncthreads();
    if (k >= Nobs) return;
    double acc = 0.0;
    for (int v = 0; v < a.nvar; v++) {
        const double *G = a.G[var * a.nvar + v] + k;
        const double *sl = s_slip + v * P;
        int64_t p = 0;
        double ga[16], gb[16];
        const int64_t nfull = P / 16;
        if (nfull > 0) {
#pragma unroll
            for (int u = 0; u < 16; u++) ga[u] = G[u * Nobs];
        }
        for (int64_t ch = 0; ch < nfull; ch += 2) {
            if (ch + 1 < nfull) {
#pragma unroll
                for (int u = 0; u < 16; u++) gb[u] = G[(p + 16 + u) * Nobs];
            }
#pragma unroll
            for (int u = 0; u < 16; u++) acc = fma(ga[u], sl[p + u], acc);
            p += 16;
            if (ch + 1 < nfull) {
                if (ch + 2 < nfull) {
#pragma unroll
                    for (int u = 0; u < 16; u++) ga[u] = G[(p + 16 + u) * Nobs];
                }
#pragma unroll
                for (int u = 0; u < 16; u++) acc = fma(gb[u], sl[p + u], acc);
                p += 16;
            }
        }
        for (; p < P; p++) acc = fma(G[p * Nobs], sl[p], acc);
    }
    a.X[var * Nobs + k] = acc;
}

int launch_crust_stack(beatamd_ctx *ctx, const double *const *G, int64_t K, int nvar, int64_t P, int64_t Nobs,
                       const double *slips, double *X)
{
    if (K == 0 || Nobs == 0) return BEATAMD_OK;
    const size_t lds = (size_t)nvar * P * sizeof(double);
    BA_CHECK(lds <= 64 * 1024, BEATAMD_EINVAL, "geo_ensemble_stack: more than 8192 patch slips (%d variables of %lld patches)",
             nvar, (long long)P);
    BA_CHECK(K <= 65535, BEATAMD_EINVAL, "geo_ensemble_stack: at most 65535 library variants");
    CrustStackArgs a;
    a.G = G; a.slips = slips; a.nvar = nvar; a.P = P; a.Nobs = Nobs; a.X = X;
    ScopedTimer tm(ctx, "cruststack");
    hipLaunchKernelGGL(k_crust_stack, dim3((unsigned)((Nobs + 127) / 128), (unsigned)K), dim3(128), lds, ctx->stream, a);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// numpy.cov(X, rowvar=0) per dataset (geodetic.py:1187), in a fixed order that a numpy restatement reproduces bit for
// bit (tests/predcov_ref.py): plain products and sums (contraction off), true divisions.
//     mean_j = (sum_k X[k,j]) / K                   k ascending, the sum starting at 0
//     D[k,j] = X[k,j] - mean_j
// Lane <-> column, eight rows' loads in flight; X is read twice (the second time from L2).
constexpr int PC_ROWS = 8;

__global__ void __launch_bounds__(256) k_pred_center(int64_t K, int64_t Nobs, const double *X, double *D)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= Nobs) return;
    const double *x = X + j;
    double s = 0.0;
    for (int64_t k0 = 0; k0 < K; k0 += PC_ROWS) {
        double v[PC_ROWS];
#pragma unroll
        for (int u = 0; u < PC_ROWS; u++) v[u] = x[(k0 + u < K ? k0 + u : K - 1) * Nobs];   // (behind the last row: not used)
#pragma unroll
        for (int u = 0; u < PC_ROWS; u++)
            if (k0 + u < K) s = s + v[u];
    }
    const double mean = s / (double)K;
    for (int64_t k0 = 0; k0 < K; k0 += PC_ROWS) {
        double v[PC_ROWS];
#pragma unroll
        for (int u = 0; u < PC_ROWS; u++) v[u] = x[(k0 + u < K ? k0 + u : K - 1) * Nobs];
#pragma unroll
        for (int u = 0; u < PC_ROWS; u++)
            if (k0 + u < K) D[(k0 + u) * Nobs + j] = v[u] - mean;
    }
}

//     out_i[a,b] = base_i[a,b] + (sum_k D[k, o_i + a] * D[k, o_i + b]) / (K - 1)     k ascending, the sum starting at 0
// Block <-> one PC_TILE x PC_TILE tile of one dataset (blockIdx.z; a block whose tile lies outside its dataset leaves at
// once), thread <-> 4 x 4 outputs.  The two operand tiles of D pass through LDS in chunks of PC_KC rows, so any K is taken;
// the accumulators carry over the chunks: one k order.  a * b == b * a, so the sums of (a,b) and (b,a) are the same
// number and the output is exactly symmetric where base_i is.  Vector FP64: n^2 K multiply-adds against the 2 n^2 8
// bytes of base and out -- bound by the matrix it reads and writes.  base == nullptr: zeros.
constexpr int PC_TILE = 64, PC_KC = 32;

__global__ void __launch_bounds__(256) k_pred_cov(int64_t K, int64_t Nobs, const double *D, const PredCovSet *sets)
{
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double sA[PC_KC][PC_TILE];
    __shared__ __attribute__((aligned(16))) double sB[PC_KC][PC_TILE];
    const PredCovSet s = sets[blockIdx.z];
    const int64_t a0 = (int64_t)blockIdx.y * PC_TILE, b0 = (int64_t)blockIdx.x * PC_TILE;
    if (a0 >= s.n || b0 >= s.n) return;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
    const double *Da = D + s.off + a0, *Db = D + s.off + b0;
    for (int64_t k0 = 0; k0 < K; k0 += PC_KC) {
        const int kc = (int)(K - k0 < PC_KC ? K - k0 : PC_KC);
#pragma unroll
        for (int i = 0; i < PC_KC * PC_TILE / 256; i++) {
            const int e = tid + 256 * i, kk = e >> 6, c = e & 63;
            const bool row = kk < kc;
            sA[kk][c] = (row && a0 + c < s.n) ? Da[(k0 + kk) * Nobs + c] : 0.0;
            sB[kk][c] = (row && b0 + c < s.n) ? Db[(k0 + kk) * Nobs + c] : 0.0;
        }
        __syncthreads();
        for (int kk = 0; kk < kc; kk++) {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { a[i] = sA[kk][ty * 4 + i]; b[i] = sB[kk][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = acc[i][j] + a[i] * b[j];
        }
        __syncthreads();
    }
    const double km1 = (double)(K - 1);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int64_t r = a0 + ty * 4 + i;
        if (r >= s.n) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t c = b0 + tx * 4 + j;
            if (c >= s.n) continue;
            const double base = s.base ? s.base[r * s.n + c] : 0.0;
            s.out[r * s.n + c] = base + acc[i][j] / km1;
        }
    }
}

// D [K, Nobs] device scratch of the caller; sets: device table of nd datasets whose sizes add up to Nobs, nmax the largest
int launch_pred_covariance(beatamd_ctx *ctx, int64_t K, int64_t Nobs, const double *X, double *D, int64_t nd, int64_t nmax,
                           const PredCovSet *sets)
{
    if (nd == 0 || Nobs == 0) return BEATAMD_OK;
    BA_CHECK(K >= 2, BEATAMD_EINVAL, "pred_covariance: a sample covariance needs at least 2 variants, got %lld", (long long)K);
    const int64_t nt = (nmax + PC_TILE - 1) / PC_TILE;
    BA_CHECK(nd <= 65535 && nt <= 65535, BEATAMD_EINVAL, "pred_covariance: at most 65535 datasets of at most %d points",
             65535 * PC_TILE);
    {
        ScopedTimer tm(ctx, "predcenter");
        hipLaunchKernelGGL(k_pred_center, dim3((unsigned)((Nobs + 255) / 256)), dim3(256), 0, ctx->stream, K, Nobs, X, D);
        BA_HIP(hipGetLastError());
    }
    ScopedTimer tm(ctx, "predcov");
    hipLaunchKernelGGL(k_pred_cov, dim3((unsigned)nt, (unsigned)nt, (unsigned)nd), dim3(256), 0, ctx->stream, K, Nobs,
                       (const double *)D, sets);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
