// geometry.hip -- analytic half-space forward models for the geometry-mode geodetic composite
// (BASELINE configs 1 and 2), batched over chains: rectangular dislocation (Okada 1985, surface
// displacements, eqs 25-30) and Mogi point source, projected on the line of sight.
//
// Reference seam: GeodeticGeometryComposite.get_formula (beat/models/geodetic.py:605-659):
//   disp = get_synths(input_rvs)            -> heart.geo_synthetics -> pyrocko engine (NOT in tree)
//   los_disp = (disp * los_vectors).sum(1)  geodetic.py:642
//   residuals = (data - los_disp) * odws ; multivariate_normal_chol
// The displacement arithmetic of the reference lives in pyrocko's GF-store engine (layered
// medium): parity with BEAT is unpinned there.  This kernel is the homogeneous
// half-space counterpart, pinned to the published check values of Okada (1985) Table 2.
//
// Work: C chains x Nobs points x nsrc sources, four corner terms (two arc tangents, two square roots,
// one division, ~60 multiply-adds each) + two logarithms per evaluation -> bound by the fp64 VALU;
// one thread per (chain, observation point), the per-(chain, source) trigonometry shared through LDS.
// The source arithmetic itself (source_const, source_disp) is in okada.hpp, shared with geolib.hip.
#include "kernels.hpp"
#include "okada.hpp"

namespace beatamd {

// one thread per (chain, observation point), flat index.  A workgroup touches the chains
// c_first .. c_last of its 256 indices: their source constants are computed once (one thread per
// (chain, source)) into LDS.  With `res` the residual of the likelihood is written instead of the
// synthetics: res = (data - mu) * odw (geodetic.py:1072-1074 / 642-650).
constexpr int GL_MAXC = 48;

// SHARED = false: more (chain, source) pairs per workgroup than the LDS table holds (very few observation
// points): every thread computes its own source constants
// CORR = true: the datasets' correction terms are subtracted in the residual epilogue (geodetic.py:1076-1077); a
// template parameter so that the instances of a model without terms are the code they were (register budget: DESIGN 3.1c)
template <int WAVES, bool SHARED, bool CORR>
__global__ void __launch_bounds__(256, WAVES) k_geom_los(GeomSrcArgs a)
{
    __shared__ SrcConst sc[SHARED ? GL_MAXC : 1];
    const int64_t total = a.C * a.Nobs;
    const int64_t i0 = (int64_t)blockIdx.x * 256;
    const int64_t i = i0 + threadIdx.x;
    const int64_t c_first = i0 / a.Nobs;
    const int64_t c_last = (min(i0 + 255, total - 1)) / a.Nobs;
    const int ncs = (int)(c_last - c_first + 1) * a.nsrc;
    if (SHARED) {
        if ((int)threadIdx.x < ncs) {
            const int cc = threadIdx.x / a.nsrc, s = threadIdx.x - cc * a.nsrc;
            source_const(a, a.Q + (c_first + cc) * a.nparams, s, sc[threadIdx.x]);
        }
        __syncthreads();
    }
    if (i >= total) return;
    const int64_t c = i / a.Nobs, k = i - c * a.Nobs;
    const double e = a.east[k], n = a.north[k];
    double ue = 0.0, un = 0.0, uz = 0.0;
    for (int s = 0; s < a.nsrc; s++) {
        double se, sn, sz;
        if (SHARED) {
            source_disp(sc[(int)(c - c_first) * a.nsrc + s], a.nu, e, n, se, sn, sz);
        } else {
            SrcConst own;
            source_const(a, a.Q + c * a.nparams, s, own);
            source_disp(own, a.nu, e, n, se, sn, sz);
        }
        ue += se;
        un += sn;
        uz += sz;
    }
    // geodetic.py:642: los_disp = (disp * los_vectors).sum(axis=1) with disp = [n, e, up]
    // (heart.py:4220-4224) and los = [Sn, Se, Su] (heart.py:1381-1410)
    const double *l = a.los + k * 3;
    const double mu = (un * l[0] + ue * l[1]) + uz * l[2];
    if (CORR)
        a.res[i] = geo_corrected_residual(a.corr, a.Q, a.nparams, c, k, a.data[k], mu, a.odw[k]);
    else if (a.res)
        a.res[i] = (a.data[k] - mu) * a.odw[k];
    else
        a.mu[i] = mu;
}

// heart.geo_synthetics (heart.py:4158-4239) for the half-space engine: one (n, e, up) array per
// (parameter set, source, observation point): out[((c*nsrc + s)*Nobs + k)*3 + {0,1,2}]
__global__ void __launch_bounds__(256) k_geom_disp(GeomSrcArgs a, double *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.C * a.nsrc * a.Nobs) return;
    const int64_t k = i % a.Nobs;
    const int64_t cs = i / a.Nobs;
    const int s = (int)(cs % a.nsrc);
    const int64_t c = cs / a.nsrc;
    double ue, un, uz;
    SrcConst own;
    source_const(a, a.Q + c * a.nparams, s, own);
    source_disp(own, a.nu, a.east[k], a.north[k], ue, un, uz);
    out[i * 3 + 0] = un;
    out[i * 3 + 1] = ue;
    out[i * 3 + 2] = uz;   // up = -down (heart.py:4222)
}

int launch_geom_disp(beatamd_ctx *ctx, int nsrc, const int32_t *kind, const int64_t *poff,
                     const double *params, int64_t C, int64_t nobs, const double *east,
                     const double *north, double nu, double *out)
{
    if (C == 0 || nobs == 0 || nsrc == 0) return BEATAMD_OK;
    GeomSrcArgs a;
    a.nsrc = nsrc; a.kind = kind; a.poff = poff; a.pfix = params;   // every slot comes from `params`
    a.Q = params; a.nparams = (int64_t)nsrc * GEO_NP; a.C = C; a.Nobs = nobs;
    a.east = east; a.north = north; a.los = nullptr; a.nu = nu; a.mu = nullptr;
    a.data = a.odw = nullptr; a.res = nullptr;
    const int64_t n = C * nsrc * nobs;
    hipLaunchKernelGGL(k_geom_disp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, a, out);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_geom_los(beatamd_ctx *ctx, const GeomSources &g, const double *Q, int64_t nparams,
                    int64_t C, double *mu, const double *data, const double *odw, double *res, GeoCorr gc)
{
    if (C == 0) return BEATAMD_OK;
    BA_CHECK(gc.nterm == 0 || (res && C <= 2147483647), BEATAMD_EINVAL,
             "geom_los: corrections act on the residual, of fewer than 2^31 chains");
    GeomSrcArgs a;
    a.nsrc = g.nsrc; a.kind = g.kind.get(); a.poff = g.poff.get(); a.pfix = g.pfix.get();
    a.Q = Q; a.nparams = nparams; a.C = C; a.Nobs = g.Nobs;
    a.east = g.east.get(); a.north = g.north.get(); a.los = g.los.get(); a.nu = g.nu; a.mu = mu;
    a.data = data; a.odw = odw; a.res = res; a.corr = gc;
    const int64_t n = C * g.Nobs;
    ScopedTimer tm(ctx, "geomlos");
    // waves per SIMD the register budget is cut for (the corner terms are long dependent fp64 chains)
    static const int waves = getenv("BEATAMD_GEOM_WAVES") ? atoi(getenv("BEATAMD_GEOM_WAVES")) : 2;
    const dim3 grid((unsigned)((n + 255) / 256));
    // chains a workgroup of 256 (chain, point) pairs can touch, times the sources
    const int64_t ncs_max = ((255 + g.Nobs - 1) / g.Nobs + 1) * g.nsrc;
    static const bool force_own = getenv("BEATAMD_GEOM_OWN") != nullptr;
    const bool corr = gc.nterm > 0;
#define GEOM_LOS(W, S)                                                                                   \
    do {                                                                                                 \
        if (corr) hipLaunchKernelGGL((k_geom_los<W, S, true>), grid, dim3(256), 0, ctx->stream, a);      \
        else hipLaunchKernelGGL((k_geom_los<W, S, false>), grid, dim3(256), 0, ctx->stream, a);          \
    } while (0)
    if (ncs_max > GL_MAXC || force_own) GEOM_LOS(2, false);
    else if (waves >= 4) GEOM_LOS(4, true);
    else if (waves == 3) GEOM_LOS(3, true);
    else GEOM_LOS(2, true);
#undef GEOM_LOS
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
