// geolib.hip -- the geodetic Green's-function library of a finite fault filled on the device.
//
// Reference seam: geo_construct_gf_linear / geo_construct_gf_linear_patches with _process_patch_geodetic
// (beat/ffi/base.py:804-1002): for every patch of unit slip in the direction of a slip component
//     disp     = heart.geo_synthetics(engine, targets, [patch], "stacked_array")      one engine call per patch
//     los_disp = (disp * los_vectors).sum(axis=1) * odws                              base.py:813
//     gfs.put(los_disp, patchidx)
// one process-pool task per patch.  Here every (component, patch) row of a launch is one source of unit slip whose
// ten kernel parameters the host states (beat_amd/discretization.py: rake, opening_fraction of the component) and
//     G[row][obs] = (u_n S_n + u_e S_e + u_u S_u) * odw
// is written straight into the device library by ONE kernel: one workgroup per (row, block of observation points),
// the row's source constants (six sin / cos, the slip decomposition) computed once by thread 0 and kept in LDS,
// one thread per observation point.  The displacement arithmetic is okada.hpp's, the text geometry.hip compiles:
// the half space of HalfspaceEngine, not the reference's layered-medium engine (parity unpinned).
#include "kernels.hpp"
#include "okada.hpp"

namespace beatamd {

struct GeoLibArgs {
    GeomSrcArgs src;       // kind / poff: one rectangular source whose ten slots are the row's parameters
    int64_t nrows, nxb;    // rows of the launch; workgroups per row
    const double *odw;     // [Nobs]
    double *G;             // [nrows, Nobs]
};

__global__ void __launch_bounds__(256, 2) k_geo_gf_library(GeoLibArgs a)
{
    __shared__ SrcConst sc;
    const int64_t row = blockIdx.x / a.nxb;          // < nrows by the grid's size
    const int64_t xb = blockIdx.x - row * a.nxb;
    if (threadIdx.x == 0) source_const(a.src, a.src.Q + row * GEO_NP, 0, sc);
    __syncthreads();
    const int64_t k = xb * blockDim.x + threadIdx.x;
    if (k >= a.src.Nobs) return;
    double ue, un, uz;
    source_disp(sc, a.src.nu, a.src.east[k], a.src.north[k], ue, un, uz);
    // base.py:813 with disp = [n, e, up] (heart.py:4220-4224) and los = [Sn, Se, Su]; numpy sums the three
    // products from the left
    const double *l = a.src.los + k * 3;
    a.G[row * a.src.Nobs + k] = ((un * l[0] + ue * l[1]) + uz * l[2]) * a.odw[k];
}

// params [nrows, 10] (device), kind / poff (device): one rectangular source with identity offsets
int launch_geo_gf_library(beatamd_ctx *ctx, int64_t nrows, const double *params, const int32_t *kind,
                          const int64_t *poff, int64_t nobs, const double *east, const double *north,
                          const double *los, const double *odw, double nu, double *G)
{
    if (nrows == 0 || nobs == 0) return BEATAMD_OK;
    GeoLibArgs a;
    a.src.nsrc = 1; a.src.kind = kind; a.src.poff = poff; a.src.pfix = params;
    a.src.Q = params; a.src.nparams = GEO_NP; a.src.C = nrows; a.src.Nobs = nobs;
    a.src.east = east; a.src.north = north; a.src.los = los; a.src.nu = nu; a.src.mu = nullptr;
    a.src.data = nullptr; a.src.odw = odw; a.src.res = nullptr;
    a.nrows = nrows; a.odw = odw; a.G = G;
    // a workgroup serves one row: as many wavefronts as the points need, four at the most
    const int threads = (int)std::min<int64_t>(256, (nobs + 63) / 64 * 64);
    a.nxb = (nobs + threads - 1) / threads;
    BA_CHECK(nrows * a.nxb < (int64_t)0x7fffffff, BEATAMD_EINVAL, "geo_gf_library: too many (row, point block) pairs");
    ScopedTimer tm(ctx, "geo_gf_library");
    hipLaunchKernelGGL(k_geo_gf_library, dim3((unsigned)(nrows * a.nxb)), dim3(threads), 0, ctx->stream, a);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
