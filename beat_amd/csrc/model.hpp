// model.hpp -- the model evaluator (model.cpp): what the entry points of capi.cpp call to evaluate an FfiModel.
#pragma once
#include "kernels.hpp"

namespace beatamd {

template <class T>
T *get_obj(std::vector<std::unique_ptr<T>> &v, int32_t id)
{
    if (id < 0 || (size_t)id >= v.size()) return nullptr;
    return v[id].get();
}

// "is this weight set evaluated on its band": banded operators found at weights_create and BEATAMD_QF_BAND not 0
inline bool wset_banded(beatamd_ctx *ctx, const WeightSet &w)
{
    return w.band >= 0 && w.wb && GfKnobs::get(gf_knobs(ctx).qf_band, 1) != 0;
}
// quad[c,d] = ||W_d x||^2 for one weight set, x(c,d,k) = X[c*xs_c + d*xs_d + k]
int wset_quad(beatamd_ctx *ctx, const WeightSet &w, int64_t C, const double *X, int64_t xs_c, int64_t xs_d, double *quad);

// datasets of the model = the first columns of the hyper model's misfit vector; all its columns: one per seismic dataset,
// one per geodetic dataset, one per slip variable of the Laplacian
int64_t model_ndata(const FfiModel &m);
int64_t model_nterm(const FfiModel &m);
int model_check_layout(const FfiModel &m);

// synthetics out [C, T, N] of one library at explicit start times [C, T, P], durations and slips [C, P]
int stack_all(beatamd_ctx *ctx, const SeisLib &lib, int64_t C, const double *durations, const double *starttimes,
              const double *slips, int interp, double *out);
// One builder per composite, used by the likelihood and by the entry points that evaluate a part of the model.
// the bad-chain flags cleared and the rupture start times of every chain: *st0 [C, P], *chain_bad [C] (scratch slots)
int model_start_times(beatamd_ctx *ctx, const FfiModel &m, int64_t C, const double *Q, double **st0, int32_t **chain_bad);
// the stacking call of one wavemap up to what its caller wants of it (mode, outputs, weights, active)
int wavemap_call(beatamd_ctx *ctx, const FfiModel &m, const Wavemap &wm, int64_t C, const double *Q, const double *st0,
                 int32_t *chain_bad, GfStackCall *k);
// geodetic synthetics mu_out [C, Nobs] and weighted, corrected residuals res_out [C, Nobs] (geometry mode writes only the
// residuals).  res_out == nullptr: the synthetics alone.  Q == nullptr: one chain of (d - 0) * odw, without corrections
int geodetic_residual(beatamd_ctx *ctx, const FfiModel &m, int64_t C, const double *Q, double *mu_out, double *res_out);
// *gc = the composite's correction table for a kernel launched next on C chains: with pole terms their derived
// coefficients are computed first (k_pole_coef) into the composite's own buffer, grown here outside any capture
int geo_pole_coefficients(beatamd_ctx *ctx, const Geodetic &g, int64_t C, const double *Q, int64_t np, GeoCorr *gc);
// the polarity composite's launch arguments up to mode, out, ld and active
void polarity_call(const Polarity &p, int64_t C, const double *Q, int64_t np, PolArgs *a);
// quad[c, v] = |L s_{c,v}|^2 of the slips [C, nvar, P]
int laplacian_quad(beatamd_ctx *ctx, const Laplacian &lap, int64_t C, int64_t nvar, const double *slips, double *quad);

// what remains after the composites wrote their columns: the `like` sum (the Metropolis step folds it into its accept kernel)
struct LikeTail {
    LikeGroups grp;
    const int32_t *chain_bad = nullptr;
};
struct LogpOpts {
    LikeTail *tail = nullptr;          // the caller sums `like` itself: it gets the composite boundaries and the bad-chain flags
    const int32_t *active = nullptr;   // device [C]: rows of LL of chains with 0 are never read; kernels may skip those chains
    double *llks = nullptr;            // device [C, nterm]: the hyper model's cached misfits instead of LL, which is not written
};
// logp_forw_func on device pointers
int ffi_logp_device(beatamd_ctx *ctx, FfiModel &m, int64_t C, const double *Q, double *LL, const LogpOpts &opt = LogpOpts());

// |W_k d_k|^2 of every dataset of the model: wset_quad on the model's own data as a one-chain batch (the geodetic data with
// its odw factor, as the residual carries it), kept on the model until drop_obs_quads
int model_obs_quads(beatamd_ctx *ctx, FfiModel &m);
void drop_obs_quads(beatamd_ctx *ctx);

// lsq start (problems.py:753-873): the normal equations N [C,P,P], b [C,P] of the chains' linear slip problems (device
// pointers); *chain_bad (a scratch slot): chains whose times leave the library grid
int lsq_normal_device(beatamd_ctx *ctx, FfiModel &m, int64_t C, const double *Q, double *Nmat, double *b, int32_t **chain_bad);

// proposal source of a step: rows handed in (delta, log_u) or drawn here (factor / scales + Philox key)
struct StepDraw {
    const double *factor = nullptr;   // [K, np] or the per-parameter scales [np]
    int64_t K = 0;
    int32_t kind = -1, df = 0;
    uint64_t seed = 0, first_chain = 0;
    uint32_t step = 0;
    int64_t groups = 1;               // multivariate: factor [groups, K, np], chain c draws with factor c / (C / groups)
};
// (groups > 1: factor [groups, K, np], the chains in `groups` equal runs, one factor each)
// delta [C, np] = z . factor for z ~ N(0, 1) [C, K] drawn here, the rows scaled to multivariate t for df > 0; log_u [C] nullable
int draw_multivariate(beatamd_ctx *ctx, int64_t C, int64_t K, int64_t np, const double *factor, int df, uint64_t seed,
                      uint32_t step, uint64_t first_chain, double *delta, double *log_u, int64_t groups = 1);
int astep_impl(beatamd_ctx *ctx, FfiModel &m, int64_t C, double *Q0, double *L0, const double *delta, const double *scaling,
               const double *lower, const double *upper, const double *log_u, double beta, const double *betas,
               int32_t *accepted, const StepDraw *draw = nullptr, int32_t *acc_sum = nullptr, int64_t *n_acc = nullptr);

}  // namespace beatamd
