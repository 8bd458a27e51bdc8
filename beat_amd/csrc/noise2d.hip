// noise2d.hip -- the 2-d neighbourhood statistic of the geodetic "non-toeplitz" noise structure (covariance.py:774-811
// k_nearest_neighbor_rms, max_dist_perc branch): per point the sample standard deviation of the data over all points of
// its dataset within a radius that is a fraction of the dataset's largest point distance.  The reference builds an
// (n, n, 2) distance temporary and asks a KD-tree once per point; here every dataset of a composite goes through three
// launches.  What follows the statistic (autocovariance, scaled Toeplitz, factorisation) is logp.hip's and chol.hip's.
#include "kernels.hpp"
#include "wave.hpp"

namespace beatamd {

// The ONE order of this file (tests/noise2d_ref.py restates it bit for bit).  Per dataset of n points, contraction off:
//     d2(i,j) = dx*dx + dy*dy,  dx = x_i - x_j, dy = y_i - y_j
//     radius  = sqrt(max_ij d2) * max_dist_perc          (sqrt correctly rounded; a maximum has no order)
//     j is a neighbour of i  iff  d2(i,j) <= radius*radius              (i is its own neighbour)
//     a sum over the neighbours of i: lane l = 0..63 adds the terms of the neighbours j == l (mod 64), j ascending, to a
//     partial that starts at 0; then partial[l] = partial[l] + partial[l + h] for l < h, h = 32, 16, 8, 4, 2, 1; the sum
//     is partial[0]
//     mean = (sum of x_j) / count;  stds[i] = sqrt((sum of (x_j - mean) * (x_j - mean)) / (count - 1));  count < 2: NaN
// It depends on (i, n) alone: one wavefront owns one point and walks the whole dataset, whatever the grid and whichever
// datasets share the call.
//
// Block <-> NB_WAVES points of ONE dataset (blockIdx.y; a block behind its dataset's last point leaves at once), wavefront
// <-> point.  The dataset passes through LDS in tiles of NB_TILE points (east, north, value: 24 KiB), so n is not bounded
// by LDS; NB_TILE is a multiple of 64, so lane l meets j == l (mod 64) in ascending order across the tiles.
constexpr int NB_WAVES = 4, NB_THREADS = NB_WAVES * 64, NB_TILE = 1024;

// tile [j0, j0 + NB_TILE) of the dataset -> LDS (behind the dataset's end: not read)
__device__ __forceinline__ void ball_stage(const BallSet s, int64_t j0, const double *coords, const double *data, double *sx,
                                           double *sy, double *sd)
{
    for (int t = threadIdx.x; t < NB_TILE; t += NB_THREADS) {
        const int64_t j = j0 + t;
        if (j < s.n) {
            sx[t] = coords[2 * (s.off + j)];
            sy[t] = coords[2 * (s.off + j) + 1];
            if (data) sd[t] = data[s.off + j];
        }
    }
}

// pmax[off + i] = max_j d2(i,j)
__global__ void __launch_bounds__(NB_THREADS) k_ball_maxd2(const BallSet *sets, const double *coords, double *pmax)
{
#pragma clang fp contract(off)
    __shared__ double sx[NB_TILE], sy[NB_TILE];
    const BallSet s = sets[blockIdx.y];
    if ((int64_t)blockIdx.x * NB_WAVES >= s.n) return;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * NB_WAVES + (threadIdx.x >> 6);
    const bool live = i < s.n;
    const double xi = live ? coords[2 * (s.off + i)] : 0.0, yi = live ? coords[2 * (s.off + i) + 1] : 0.0;
    double m = 0.0;
    for (int64_t j0 = 0; j0 < s.n; j0 += NB_TILE) {
        ball_stage(s, j0, coords, nullptr, sx, sy, nullptr);
        __syncthreads();
        const int nt = (int)(s.n - j0 < NB_TILE ? s.n - j0 : NB_TILE);
        for (int t = lane; t < nt; t += 64) {
            const double dx = xi - sx[t], dy = yi - sy[t];
            const double d2 = dx * dx + dy * dy;
            m = d2 > m ? d2 : m;
        }
        __syncthreads();
    }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {   // wave_tree<OpSelGreater> (wave.hpp); the call changes the generated code
        const double o = __shfl_down(m, h, 64);
        m = o > m ? o : m;
    }
    if (live && lane == 0) pmax[s.off + i] = m;
}

// radius[d] = sqrt(max_i pmax[off_d + i]) * max_dist_perc; one block per dataset
__global__ void __launch_bounds__(NB_THREADS) k_ball_radius(const BallSet *sets, const double *pmax, double max_dist_perc,
                                                            double *radius)
{
#pragma clang fp contract(off)
    __shared__ double sm[NB_THREADS];
    const BallSet s = sets[blockIdx.x];
    double m = 0.0;
    for (int64_t i = threadIdx.x; i < s.n; i += NB_THREADS) {
        const double v = pmax[s.off + i];
        m = v > m ? v : m;
    }
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int h = NB_THREADS / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) sm[threadIdx.x] = sm[threadIdx.x + h] > sm[threadIdx.x] ? sm[threadIdx.x + h] : sm[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) radius[blockIdx.x] = __dsqrt_rn(sm[0]) * max_dist_perc;
}

// counts[off + i], stds[off + i]: two passes over the dataset's tiles (mean, then squared deviations); the neighbour test
// is evaluated again in the second pass -- the same operations on the same numbers, the same set
__global__ void __launch_bounds__(NB_THREADS) k_ball_rms(const BallSet *sets, const double *coords, const double *data,
                                                         const double *radius, int32_t *counts, double *stds)
{
#pragma clang fp contract(off)
    __shared__ double sx[NB_TILE], sy[NB_TILE], sd[NB_TILE];
    const BallSet s = sets[blockIdx.y];
    if ((int64_t)blockIdx.x * NB_WAVES >= s.n) return;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * NB_WAVES + (threadIdx.x >> 6);
    const bool live = i < s.n;
    const double xi = live ? coords[2 * (s.off + i)] : 0.0, yi = live ? coords[2 * (s.off + i) + 1] : 0.0;
    const double r = radius[blockIdx.y];
    const double r2 = r * r;
    double mean = 0.0, acc = 0.0;
    int cnt = 0;
    for (int pass = 0; pass < 2; pass++) {
        acc = 0.0;
        for (int64_t j0 = 0; j0 < s.n; j0 += NB_TILE) {
            ball_stage(s, j0, coords, data, sx, sy, sd);
            __syncthreads();
            const int nt = (int)(s.n - j0 < NB_TILE ? s.n - j0 : NB_TILE);
            for (int t = lane; t < nt; t += 64) {
                const double dx = xi - sx[t], dy = yi - sy[t];
                const double d2 = dx * dx + dy * dy;
                if (d2 <= r2) {
                    if (pass == 0) {
                        acc = acc + sd[t];
                        cnt++;
                    } else {
                        const double e = sd[t] - mean;
                        acc = acc + e * e;
                    }
                }
            }
            __syncthreads();
        }
        acc = wave_tree_bcast<OpAdd>(acc);   // the halving tree of the order above, lane 0's sum in every lane
        if (pass == 0) {
            cnt = wave_tree_bcast<OpAdd>(cnt);
            mean = acc / (double)cnt;
        }
    }
    if (live && lane == 0) {
        counts[s.off + i] = cnt;
        stds[s.off + i] = cnt < 2 ? __builtin_nan("") : __dsqrt_rn(acc / (double)(cnt - 1));
    }
}

// sets: device table of nd datasets, nmax the largest; pmax [Ntot] device scratch of the caller
int launch_ball_rms(beatamd_ctx *ctx, int64_t nd, int64_t nmax, const BallSet *sets, const double *coords, const double *data,
                    double max_dist_perc, double *pmax, double *radius, int32_t *counts, double *stds)
{
    if (nd == 0 || nmax == 0) return BEATAMD_OK;
    const int64_t nb = (nmax + NB_WAVES - 1) / NB_WAVES;
    BA_CHECK(nd <= 65535 && nb <= 2147483647, BEATAMD_EINVAL, "ball_rms_batch: at most 65535 datasets");
    ScopedTimer tm(ctx, "ballrms");
    const dim3 grid((unsigned)nb, (unsigned)nd);
    hipLaunchKernelGGL(k_ball_maxd2, grid, dim3(NB_THREADS), 0, ctx->stream, sets, coords, pmax);
    BA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ball_radius, dim3((unsigned)nd), dim3(NB_THREADS), 0, ctx->stream, sets, (const double *)pmax,
                       max_dist_perc, radius);
    BA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ball_rms, grid, dim3(NB_THREADS), 0, ctx->stream, sets, coords, data, (const double *)radius, counts,
                       stds);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
