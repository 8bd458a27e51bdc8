// capi.cpp -- the extern "C" entry points of include/beat_amd.h (host side of the engine).
#include <cstdlib>

#include "model.hpp"

using namespace beatamd;

namespace {

template <class T>
int32_t add_obj(std::vector<std::unique_ptr<T>> &v, std::unique_ptr<T> o)
{
    for (size_t i = 0; i < v.size(); i++)
        if (!v[i]) {
            v[i] = std::move(o);
            return (int32_t)i;
        }
    v.push_back(std::move(o));
    return (int32_t)v.size() - 1;
}

// host copy of a small argument array that may live on either side
template <class T>
int host_copy(beatamd_ctx *ctx, const T *p, size_t n, std::vector<T> &out)
{
    out.resize(n);
    if (n == 0) return BEATAMD_OK;
    if (is_device_ptr(p)) {
        BA_HIP(hipMemcpyAsync(out.data(), p, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        BA_HIP(hipStreamSynchronize(ctx->stream));
    } else {
        memcpy(out.data(), p, n * sizeof(T));
    }
    return BEATAMD_OK;
}

#define ENTER(ctx)                                                    \
    BA_CHECK((ctx) != nullptr, BEATAMD_EINVAL, "ctx is NULL");        \
    BA_HIP(hipSetDevice((ctx)->device))

// ---- object lookups: the id's object, or EINVAL with the message that callers match on
template <class T>
int find_obj(std::vector<std::unique_ptr<T>> &v, int32_t id, const char *what, T **out)
{
    *out = get_obj(v, id);
    BA_CHECK(*out, BEATAMD_EINVAL, "unknown %s %d", what, id);
    return BEATAMD_OK;
}
// *_destroy: drain the stream, then the object goes and frees its device arrays
template <class T>
int destroy_obj(beatamd_ctx *ctx, std::vector<std::unique_ptr<T>> &v, int32_t id, const char *what)
{
    T *o;
    BA_TRY(find_obj(v, id, what, &o));
    BA_HIP(hipStreamSynchronize(ctx->stream));
    v[id].reset();
    return BEATAMD_OK;
}
int find_model(beatamd_ctx *ctx, int32_t id, FfiModel **m) { return find_obj(ctx->models, id, "model", m); }
int find_wset(beatamd_ctx *ctx, int32_t id, WeightSet **w) { return find_obj(ctx->wsets, id, "weight set", w); }
int find_seislib(beatamd_ctx *ctx, int32_t id, SeisStore **l) { return find_obj(ctx->seislibs, id, "GF library", l); }
int find_geolib(beatamd_ctx *ctx, int32_t id, GeoLib **l) { return find_obj(ctx->geolibs, id, "geodetic GF library", l); }
int find_lap(beatamd_ctx *ctx, int32_t id, Laplacian **l) { return find_obj(ctx->laps, id, "laplacian", l); }
int find_hyper(beatamd_ctx *ctx, int32_t id, HyperModel **h) { return find_obj(ctx->hypers, id, "hyper model", h); }

// *flag: every matrix of the stack W [nd, M, M] has exact zeros below its diagonal (one host synchronisation)
int upper_tri_flag(beatamd_ctx *ctx, const double *W, int64_t nd, int64_t M, int *flag)
{
    int *d_flag;
    BA_TRY(ctx->scratch(SL_MISC, 16, &d_flag));
    BA_TRY(launch_check_upper_tri(ctx, W, nd, M, d_flag));
    BA_HIP(hipMemcpyAsync(flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    BA_HIP(hipStreamSynchronize(ctx->stream));
    return BEATAMD_OK;
}

// sum and maximum of the `which`-th per-(group, target, patch) counter array of the most recent chain-shared launch
int gs_counters(beatamd_ctx *ctx, int which, int64_t *total, int64_t *max)
{
    BA_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<uint32_t> n((size_t)ctx->gs_ngtp);
    BA_HIP(hipMemcpy(n.data(), (const uint32_t *)ctx->scratch_bufs[SL_GS_UCOUNT].p + which * ctx->gs_ngtp,
                     n.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *total = *max = 0;
    for (uint32_t u : n) {
        *total += u;
        *max = std::max<int64_t>(*max, u);
    }
    return BEATAMD_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ fast sweep
int beatamd_fast_sweep_batch(beatamd_ctx *ctx, const double *slowness, double patch_size,
                             const int32_t *h_strk, const int32_t *h_dip, int32_t num_strk,
                             int32_t num_dip, int64_t C, double *out)
{
    ENTER(ctx);
    BA_CHECK(slowness && h_strk && h_dip && out, BEATAMD_EINVAL, "fast_sweep: NULL array");
    BA_CHECK(num_strk > 0 && num_dip > 0 && C >= 0, BEATAMD_EINVAL, "fast_sweep: bad dimensions");
    if (C == 0) return BEATAMD_OK;
    const int64_t n = (int64_t)num_strk * num_dip;
    Staging st(ctx);
    const double *d_s;
    const int32_t *d_hi, *d_hj;
    double *d_o;
    BA_TRY(st.in(slowness, (size_t)C * n, &d_s));
    BA_TRY(st.in(h_strk, (size_t)C, &d_hi));
    BA_TRY(st.in(h_dip, (size_t)C, &d_hj));
    BA_TRY(st.out(out, (size_t)C * n, &d_o));
    BA_TRY(launch_sweep_explicit(ctx, d_s, patch_size, d_hi, d_hj, num_strk, num_dip, C, d_o));
    return st.finish();
}

// ------------------------------------------------------------------ GF libraries
int beatamd_seis_gflib_create(beatamd_ctx *ctx, int64_t T, int64_t P, int64_t D, int64_t S,
                              int64_t N, double st_min, double st_dt, double du_min, double du_dt,
                              int32_t *lib_id)
{
    ENTER(ctx);
    BA_CHECK(lib_id, BEATAMD_EINVAL, "lib_id is NULL");
    BA_CHECK(T > 0 && P > 0 && D > 0 && S > 0 && N > 0, BEATAMD_EINVAL,
             "GF library dimensions must be positive");
    BA_CHECK(st_dt > 0 && du_dt > 0, BEATAMD_EINVAL, "sampling intervals must be positive");
    BA_CHECK(D < 32768 && S < 32768, BEATAMD_EINVAL, "int16 index range exceeded");
    std::unique_ptr<SeisStore> l(new SeisStore());
    l->T = T; l->P = P; l->D = D; l->S = S; l->N = N;
    l->st_min = st_min; l->st_dt = st_dt; l->du_min = du_min; l->du_dt = du_dt;
    *lib_id = add_obj(ctx->seislibs, std::move(l));
    return BEATAMD_OK;
}

int beatamd_seis_gflib_set_split_targets(beatamd_ctx *ctx, int32_t lib_id, int64_t ntargets)
{
    ENTER(ctx);
    SeisStore *l;
    BA_TRY(find_seislib(ctx, lib_id, &l));
    BA_CHECK(ntargets >= 0, BEATAMD_EINVAL, "gflib_set_split_targets: negative target count");
    BA_CHECK(ntargets == 0 || ntargets >= l->T, BEATAMD_EINVAL,
             "gflib_set_split_targets: %lld targets, fewer than the library's %lld", (long long)ntargets, (long long)l->T);
    l->split_T = ntargets;
    return BEATAMD_OK;
}

static int seis_ensure_storage(SeisStore *l)
{
    if (l->g) return BEATAMD_OK;
    const hipError_t e = l->own.try_alloc((size_t)l->elems());
    BA_CHECK(e == hipSuccess, BEATAMD_ENOMEM, "GF library of %.2f GB does not fit in HBM: %s",
             (size_t)l->elems() * sizeof(double) / 1e9, hipGetErrorString(e));
    l->g = l->own.get();
    return BEATAMD_OK;
}

// The float copy and the float64 storage hold the same values only as long as nobody rewrites the float64 rows:
// an upload or an in-place (re-)whitening drops the copy and takes the models' wavemaps off it.
static void drop_f32_overlapping(beatamd_ctx *ctx, const void *p, size_t bytes)
{
    const char *a = (const char *)p, *b = a + bytes;
    for (size_t id = 0; id < ctx->seislibs.size(); id++) {
        SeisStore *l = ctx->seislibs[id].get();
        if (!l || !l->g32 || !l->g) continue;
        const char *la = (const char *)l->g, *lb = la + (size_t)l->elems() * sizeof(double);
        if (b <= la || lb <= a) continue;
        (void)hipStreamSynchronize(ctx->stream);
        l->own32.reset();
        l->g32 = nullptr;
        for (auto &m : ctx->models) {
            if (!m) continue;
            for (Wavemap &w : m->wavemaps)
                for (int32_t lid : w.libs)
                    if ((size_t)lid == id) w.f32 = false;
        }
    }
}

int beatamd_seis_gflib_round_to_f32(beatamd_ctx *ctx, int32_t lib_id)
{
    ENTER(ctx);
    SeisStore *l = get_obj(ctx->seislibs, lib_id);
    BA_CHECK(l && l->g, BEATAMD_EINVAL, "gflib_round_to_f32: unknown or empty GF library %d", lib_id);
    if (!l->g32) {
        const hipError_t e = l->own32.try_alloc((size_t)l->elems());
        BA_CHECK(e == hipSuccess, BEATAMD_ENOMEM, "float copy of the GF library (%.2f GB) does not fit in HBM: %s",
                 l->elems() * 4 / 1e9, hipGetErrorString(e));
        l->g32 = l->own32.get();
    }
    BA_TRY(launch_round_to_f32(ctx, l->g, l->g32, l->elems()));
    return BEATAMD_OK;
}

int beatamd_ffi_model_set_f32(beatamd_ctx *ctx, int32_t model_id, int32_t wavemap_index, int32_t on)
{
    ENTER(ctx);
    FfiModel *m = get_obj(ctx->models, model_id);
    BA_CHECK(m && wavemap_index >= 0 && wavemap_index < (int32_t)m->wavemaps.size(), BEATAMD_EINVAL,
             "model_set_f32: unknown model / wavemap");
    Wavemap &w = m->wavemaps[wavemap_index];
    if (on)
        for (int32_t id : w.libs) {
            SeisLib *l = get_obj(ctx->seislibs, id);
            BA_CHECK(l && l->g32, BEATAMD_EINVAL,
                     "model_set_f32: library %d has no float copy (beatamd_seis_gflib_round_to_f32; an upload or a "
                     "re-whitening of its rows drops the copy)", id);
        }
    w.f32 = on != 0;
    return BEATAMD_OK;
}

int beatamd_seis_gflib_upload(beatamd_ctx *ctx, int32_t lib_id, const double *src, int64_t offset,
                              int64_t count)
{
    ENTER(ctx);
    SeisStore *l;
    BA_TRY(find_seislib(ctx, lib_id, &l));
    BA_CHECK(src && offset >= 0 && count >= 0 && offset + count <= l->elems(), BEATAMD_EINVAL,
             "gflib_upload: range [%lld, %lld) outside the library (%lld elements)",
             (long long)offset, (long long)(offset + count), (long long)l->elems());
    BA_TRY(seis_ensure_storage(l));
    drop_f32_overlapping(ctx, l->g + offset, (size_t)count * 8);
    BA_HIP(hipMemcpyAsync(l->g + offset, src, (size_t)count * 8, hipMemcpyDefault, ctx->stream));
    BA_HIP(hipStreamSynchronize(ctx->stream));
    return BEATAMD_OK;
}

int beatamd_seis_gflib_adopt(beatamd_ctx *ctx, int32_t lib_id, double *device_ptr)
{
    ENTER(ctx);
    SeisStore *l;
    BA_TRY(find_seislib(ctx, lib_id, &l));
    BA_CHECK(device_ptr && is_device_ptr(device_ptr), BEATAMD_EINVAL,
             "gflib_adopt needs a device pointer");
    BA_CHECK(((uintptr_t)device_ptr & 15) == 0, BEATAMD_EINVAL,
             "gflib_adopt: pointer must be 16-byte aligned");
    l->own.reset();
    l->own32.reset();   // (a float copy belongs to the old storage)
    l->g32 = nullptr;
    l->g = device_ptr;
    return BEATAMD_OK;
}

int beatamd_seis_gflib_device_ptr(beatamd_ctx *ctx, int32_t lib_id, double **device_ptr)
{
    ENTER(ctx);
    SeisStore *l = get_obj(ctx->seislibs, lib_id);
    BA_CHECK(l && device_ptr, BEATAMD_EINVAL, "unknown GF library %d", lib_id);
    BA_TRY(seis_ensure_storage(l));
    *device_ptr = l->g;
    return BEATAMD_OK;
}

int beatamd_seis_gflib_destroy(beatamd_ctx *ctx, int32_t lib_id)
{
    ENTER(ctx);
    return destroy_obj(ctx, ctx->seislibs, lib_id, "GF library");
}

int beatamd_seis_stack_all_batch(beatamd_ctx *ctx, int32_t lib_id, int64_t C,
                                 const double *durations, const double *starttimes,
                                 const double *slips, int32_t interpolation, double *out)
{
    ENTER(ctx);
    SeisStore *l;
    BA_TRY(find_seislib(ctx, lib_id, &l));
    BA_CHECK(l->g, BEATAMD_EINVAL, "GF library %d holds no data (upload or adopt first)", lib_id);
    BA_CHECK(durations && starttimes && slips && out, BEATAMD_EINVAL, "stack_all: NULL array");
    BA_CHECK(interpolation == BEATAMD_NEAREST_NEIGHBOR || interpolation == BEATAMD_MULTILINEAR,
             BEATAMD_EINVAL, "Interpolation scheme %d not implemented!", interpolation);
    BA_CHECK(C >= 0, BEATAMD_EINVAL, "negative batch size");
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_du, *d_st, *d_sl;
    double *d_o;
    BA_TRY(st.in(durations, (size_t)C * l->P, &d_du));
    BA_TRY(st.in(starttimes, (size_t)C * l->T * l->P, &d_st));
    BA_TRY(st.in(slips, (size_t)C * l->P, &d_sl));
    BA_TRY(st.out(out, (size_t)C * l->T * l->N, &d_o));
    BA_TRY(stack_all(ctx, *l, C, d_du, d_st, d_sl, interpolation, d_o));
    return st.finish();
}

int beatamd_geo_gflib_create(beatamd_ctx *ctx, int64_t P, int64_t Nobs, const double *G,
                             int32_t *lib_id)
{
    ENTER(ctx);
    BA_CHECK(lib_id && G && P > 0 && Nobs > 0, BEATAMD_EINVAL, "geo_gflib_create: bad argument");
    std::unique_ptr<GeoLib> l(new GeoLib());
    l->P = P;
    l->Nobs = Nobs;
    BA_TRY(l->g.alloc_copy(ctx, G, (size_t)P * Nobs));
    *lib_id = add_obj(ctx->geolibs, std::move(l));
    return BEATAMD_OK;
}

int beatamd_geo_gflib_destroy(beatamd_ctx *ctx, int32_t lib_id)
{
    ENTER(ctx);
    return destroy_obj(ctx, ctx->geolibs, lib_id, "geodetic GF library");
}

int beatamd_geo_stack_all_batch(beatamd_ctx *ctx, int32_t lib_id, int64_t C, const double *slips,
                                int32_t accumulate, double *out)
{
    ENTER(ctx);
    GeoLib *l;
    BA_TRY(find_geolib(ctx, lib_id, &l));
    BA_CHECK(slips && out && C >= 0, BEATAMD_EINVAL, "geo_stack_all: bad argument");
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_sl;
    double *d_o;
    BA_TRY(st.in(slips, (size_t)C * l->P, &d_sl));
    BA_TRY(st.out(out, (size_t)C * l->Nobs, &d_o, accumulate != 0));
    const GeoLib *one[1] = {l};
    const ChainVec sv[1] = {ChainVec{d_sl, l->P, 0}};
    BA_TRY(launch_geo_stack(ctx, one, 1, C, sv, accumulate, d_o));
    return st.finish();
}

// ------------------------------------------------------------------ velocity-model prediction covariance
int beatamd_geo_ensemble_create(beatamd_ctx *ctx, const int32_t *lib_ids, int64_t K, int64_t nvar, int32_t *ens_id)
{
    ENTER(ctx);
    BA_CHECK(lib_ids && ens_id && K >= 1 && K <= 65535 && nvar >= 1 && nvar <= 4, BEATAMD_EINVAL,
             "geo_ensemble_create: bad argument (1..65535 variants of 1..4 slip variables)");
    std::vector<int32_t> ids;
    BA_TRY(host_copy(ctx, lib_ids, (size_t)(K * nvar), ids));
    std::unique_ptr<GeoEnsemble> e(new GeoEnsemble());
    e->K = K;
    e->nvar = nvar;
    e->libs = ids;
    for (size_t i = 0; i < ids.size(); i++) {
        GeoLib *l;
        BA_TRY(find_geolib(ctx, ids[i], &l));
        if (i == 0) {
            e->P = l->P;
            e->Nobs = l->Nobs;
        }
        BA_CHECK(l->P == e->P && l->Nobs == e->Nobs, BEATAMD_EINVAL,
                 "geo_ensemble_create: library %d is (%lld, %lld), the first one (%lld, %lld)", ids[i], (long long)l->P,
                 (long long)l->Nobs, (long long)e->P, (long long)e->Nobs);
        e->ptrs.push_back(l->g.get());
    }
    BA_TRY(e->table.alloc_copy(ctx, e->ptrs.data(), e->ptrs.size()));
    *ens_id = add_obj(ctx->geoens, std::move(e));
    return BEATAMD_OK;
}

int beatamd_geo_ensemble_destroy(beatamd_ctx *ctx, int32_t ens_id)
{
    ENTER(ctx);
    return destroy_obj(ctx, ctx->geoens, ens_id, "geodetic library ensemble");
}

int beatamd_geo_ensemble_stack(beatamd_ctx *ctx, int32_t ens_id, const double *slips, double *X)
{
    ENTER(ctx);
    GeoEnsemble *e;
    BA_TRY(find_obj(ctx->geoens, ens_id, "geodetic library ensemble", &e));
    BA_CHECK(slips && X, BEATAMD_EINVAL, "geo_ensemble_stack: NULL array");
    for (size_t i = 0; i < e->libs.size(); i++) {
        const GeoLib *l = get_obj(ctx->geolibs, e->libs[i]);
        BA_CHECK(l && l->g.get() == e->ptrs[i], BEATAMD_EINVAL,
                 "geo_ensemble_stack: library %d of the ensemble was destroyed or replaced", e->libs[i]);
    }
    Staging st(ctx);
    const double *d_sl;
    double *d_x;
    BA_TRY(st.in(slips, (size_t)(e->nvar * e->P), &d_sl));
    BA_TRY(st.out(X, (size_t)(e->K * e->Nobs), &d_x));
    BA_TRY(launch_crust_stack(ctx, e->table.get(), e->K, (int)e->nvar, e->P, e->Nobs, d_sl, d_x));
    return st.finish();
}

int beatamd_pred_covariance_batch(beatamd_ctx *ctx, int64_t K, int64_t Nobs, const double *X, int64_t nd, const int64_t *sizes,
                                  const double *const *base, double *const *out)
{
    ENTER(ctx);
    BA_CHECK(X && sizes && out && Nobs >= 0 && nd >= 0, BEATAMD_EINVAL, "pred_covariance_batch: bad argument");
    BA_CHECK(K >= 2, BEATAMD_EINVAL, "pred_covariance_batch: a sample covariance needs at least 2 variants, got %lld",
             (long long)K);
    BA_CHECK(!is_device_ptr(base) && !is_device_ptr(out), BEATAMD_EINVAL,
             "pred_covariance_batch: the lists of matrix pointers are host arrays (the matrices may live on either side)");
    if (nd == 0) return BEATAMD_OK;
    std::vector<int64_t> n;
    BA_TRY(host_copy(ctx, sizes, (size_t)nd, n));
    // a matrix may live on either side: the host ones are mirrored in one array of this call (a composite has any number
    // of datasets, Staging a fixed number of slots), bases in front of the outputs
    int64_t total = 0, nmax = 0;
    size_t host_elems = 0;
    for (int64_t i = 0; i < nd; i++) {
        BA_CHECK(n[i] > 0 && out[i], BEATAMD_EINVAL, "pred_covariance_batch: dataset %lld is empty or has no output", (long long)i);
        total += n[i];
        nmax = std::max(nmax, n[i]);
        const size_t nn = (size_t)(n[i] * n[i]);
        if (base && base[i] && !is_device_ptr(base[i])) host_elems += nn;
        if (!is_device_ptr(out[i])) host_elems += nn;
    }
    BA_CHECK(total == Nobs, BEATAMD_EINVAL, "pred_covariance_batch: the dataset sizes add up to %lld, X has %lld columns",
             (long long)total, (long long)Nobs);
    DevMem<double> mirror;
    if (host_elems) BA_TRY(mirror.alloc(host_elems));
    std::vector<PredCovSet> sets((size_t)nd);
    struct Back { double *host; const double *dev; size_t bytes; };
    std::vector<Back> back;
    size_t used = 0;
    int64_t off = 0;
    for (int64_t i = 0; i < nd; i++) {
        const size_t nn = (size_t)(n[i] * n[i]);
        PredCovSet &s = sets[(size_t)i];
        s.off = off;
        s.n = n[i];
        s.base = base ? base[i] : nullptr;
        if (s.base && !is_device_ptr(s.base)) {
            BA_HIP(hipMemcpyAsync(mirror.get() + used, s.base, nn * 8, hipMemcpyHostToDevice, ctx->stream));
            s.base = mirror.get() + used;
            used += nn;
        }
        s.out = out[i];
        if (!is_device_ptr(s.out)) {
            s.out = mirror.get() + used;
            back.push_back(Back{out[i], s.out, nn * 8});
            used += nn;
        }
        off += n[i];
    }
    Staging st(ctx);
    const double *d_x;
    double *d_D;
    PredCovSet *d_sets;
    BA_TRY(st.in(X, (size_t)(K * Nobs), &d_x));
    BA_TRY(ctx->scratch(SL_PARTIAL, (size_t)(K * Nobs), &d_D));
    BA_TRY(ctx->scratch(SL_MISC, (size_t)nd, &d_sets));
    BA_HIP(hipMemcpyAsync(d_sets, sets.data(), sets.size() * sizeof(PredCovSet), hipMemcpyHostToDevice, ctx->stream));
    BA_TRY(launch_pred_covariance(ctx, K, Nobs, d_x, d_D, nd, nmax, d_sets));
    for (const Back &b : back) BA_HIP(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, ctx->stream));
    // the table and the mirror are this call's: the stream is drained before they go
    BA_HIP(hipStreamSynchronize(ctx->stream));
    return st.finish();
}

// ------------------------------------------------------------------ likelihood
static int wset_fill(beatamd_ctx *ctx, WeightSet *w, const double *weights, const double *slog)
{
    const size_t wbytes =
        (size_t)(w->kind == BEATAMD_W_SCALAR ? w->nd : w->nd * w->M * w->M) * sizeof(double);
    BA_HIP(hipMemcpyAsync(w->w.get(), weights, wbytes, hipMemcpyDefault, ctx->stream));
    BA_HIP(hipMemcpyAsync(w->slog.get(), slog, (size_t)w->nd * 8, hipMemcpyDefault, ctx->stream));
    BA_HIP(hipStreamSynchronize(ctx->stream));
    w->upper_tri = 0;
    if (w->kind == BEATAMD_W_DENSE) {
        int flag = 0;
        BA_TRY(upper_tri_flag(ctx, w->w.get(), w->nd, w->M, &flag));
        w->upper_tri = flag;
        // banded?  (upper-triangular with nothing beyond a few columns right of the diagonal)
        w->band = -1;
        w->wb.reset();
        if (flag && w->M > 2 * QF_BAND_LIMIT) {
            void *p = nullptr;   // sized in bytes on purpose: launch_band_detect lays its scratch out itself
            BA_TRY(ctx->get_scratch(SL_MISC, (size_t)w->nd * w->M * 8 + 64, &p));
            int64_t band = -1;
            w->dropped_rel = 0.0;
            BA_TRY(launch_band_detect(ctx, w->w.get(), w->nd, w->M, p, &band, &w->dropped_rel));
            // the choice is visible: beatamd_weights_band_info, and one line under BEATAMD_VERBOSE
            if (getenv("BEATAMD_VERBOSE"))
                fprintf(stderr, "beat_amd: weight set of %lld operators of %lld^2: %s (half bandwidth %lld, largest entry beyond it "
                                "%.3g of its row's largest)\n", (long long)w->nd, (long long)w->M,
                        band <= QF_BAND_LIMIT ? "evaluated on its band" : "dense", (long long)band, w->dropped_rel);
            if (band >= 0 && band <= QF_BAND_LIMIT) {
                DevMem<double> wb;
                BA_TRY(wb.alloc((size_t)(w->nd * w->M * (band + 1))));
                BA_TRY(launch_band_pack(ctx, w->w.get(), w->nd, w->M, band, wb.get()));
                w->wb = std::move(wb);
                w->band = band;
            }
        }
    }
    return BEATAMD_OK;
}

int beatamd_weights_create(beatamd_ctx *ctx, int32_t kind, int64_t nd, int64_t M,
                           const double *weights, const double *slog_pdet, int32_t *wset_id)
{
    ENTER(ctx);
    BA_CHECK(kind == BEATAMD_W_SCALAR || kind == BEATAMD_W_DENSE, BEATAMD_EINVAL,
             "unknown weight kind %d", kind);
    BA_CHECK(nd > 0 && M > 0 && weights && slog_pdet && wset_id, BEATAMD_EINVAL,
             "weights_create: bad argument");
    std::unique_ptr<WeightSet> w(new WeightSet());
    w->kind = kind;
    w->nd = nd;
    w->M = M;
    BA_TRY(w->w.alloc((size_t)(kind == BEATAMD_W_SCALAR ? nd : nd * M * M)));
    BA_TRY(w->slog.alloc((size_t)nd));
    BA_TRY(wset_fill(ctx, w.get(), weights, slog_pdet));
    *wset_id = add_obj(ctx->wsets, std::move(w));
    return BEATAMD_OK;
}

int beatamd_weights_update(beatamd_ctx *ctx, int32_t wset_id, int32_t kind, int64_t count,
                           const double *weights, const double *slog_pdet)
{
    ENTER(ctx);
    WeightSet *w = get_obj(ctx->wsets, wset_id);
    BA_CHECK(w && weights && slog_pdet, BEATAMD_EINVAL, "weights_update: bad argument");
    BA_CHECK(kind == w->kind, BEATAMD_EINVAL,
             "weights_update: weight set %d holds %s weights, got %s ones (a pre-whitened wavemap "
             "keeps scalar weights: re-whiten the library instead)", wset_id,
             w->kind == BEATAMD_W_SCALAR ? "scalar" : "dense", kind == BEATAMD_W_SCALAR ? "scalar" : "dense");
    const int64_t want = w->kind == BEATAMD_W_SCALAR ? w->nd : w->nd * w->M * w->M;
    BA_CHECK(count == want, BEATAMD_EINVAL, "weights_update: %lld elements given, the set holds %lld",
             (long long)count, (long long)want);
    BA_HIP(hipStreamSynchronize(ctx->stream));
    drop_obs_quads(ctx);
    return wset_fill(ctx, w, weights, slog_pdet);
}

int beatamd_weights_band_info(beatamd_ctx *ctx, int32_t wset_id, int64_t *band, double *max_dropped_rel)
{
    ENTER(ctx);
    WeightSet *w = get_obj(ctx->wsets, wset_id);
    BA_CHECK(w && band && max_dropped_rel, BEATAMD_EINVAL, "weights_band_info: bad argument");
    const bool on = wset_banded(ctx, *w);
    *band = on ? w->band : -1;
    *max_dropped_rel = on ? w->dropped_rel : 0.0;
    return BEATAMD_OK;
}

int beatamd_weights_band(beatamd_ctx *ctx, int32_t wset_id, int64_t *band)
{
    ENTER(ctx);
    BA_CHECK(get_obj(ctx->wsets, wset_id) && band, BEATAMD_EINVAL, "weights_band: unknown weight set %d", wset_id);
    double dropped_rel;
    return beatamd_weights_band_info(ctx, wset_id, band, &dropped_rel);
}

int beatamd_weights_destroy(beatamd_ctx *ctx, int32_t wset_id)
{
    ENTER(ctx);
    return destroy_obj(ctx, ctx->wsets, wset_id, "weight set");
}

int beatamd_mvn_chol_logp_batch(beatamd_ctx *ctx, int32_t wset_id, int64_t C,
                                const double *residuals, const double *hp, double *logpts)
{
    ENTER(ctx);
    WeightSet *w;
    BA_TRY(find_wset(ctx, wset_id, &w));
    BA_CHECK(residuals && hp && logpts && C >= 0, BEATAMD_EINVAL, "mvn_chol_logp: bad argument");
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_r, *d_h;
    double *d_o, *quad;
    BA_TRY(st.in(residuals, (size_t)C * w->nd * w->M, &d_r));
    BA_TRY(st.in(hp, (size_t)C * w->nd, &d_h));
    BA_TRY(st.out(logpts, (size_t)C * w->nd, &d_o));
    BA_TRY(ctx->scratch(SL_QUAD, (size_t)C * w->nd, &quad));
    BA_TRY(wset_quad(ctx, *w, C, d_r, w->nd * w->M, w->M, quad));
    BA_TRY(launch_mvn_finish(ctx, C, w->nd, w->M, quad, w->slog.get(), HpSrc{d_h, w->nd, nullptr}, d_o, w->nd));
    return st.finish();
}

int beatamd_laplacian_create(beatamd_ctx *ctx, int64_t P, const double *L, double logdet,
                             int32_t *lap_id)
{
    ENTER(ctx);
    BA_CHECK(P > 0 && L && lap_id, BEATAMD_EINVAL, "laplacian_create: bad argument");
    std::unique_ptr<Laplacian> l(new Laplacian());
    l->P = P;
    l->logdet = logdet;
    BA_TRY(l->L.alloc_copy(ctx, L, (size_t)P * P));
    *lap_id = add_obj(ctx->laps, std::move(l));
    return BEATAMD_OK;
}

int beatamd_laplacian_destroy(beatamd_ctx *ctx, int32_t lap_id)
{
    ENTER(ctx);
    return destroy_obj(ctx, ctx->laps, lap_id, "laplacian");
}

int beatamd_laplacian_logp_batch(beatamd_ctx *ctx, int32_t lap_id, int64_t C, int64_t nvar,
                                 const double *slips, const double *hp, double *out)
{
    ENTER(ctx);
    Laplacian *l;
    BA_TRY(find_lap(ctx, lap_id, &l));
    BA_CHECK(slips && hp && out && C >= 0 && nvar > 0, BEATAMD_EINVAL, "laplacian_logp: bad argument");
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_s, *d_h;
    double *d_o, *quad;
    BA_TRY(st.in(slips, (size_t)C * nvar * l->P, &d_s));
    BA_TRY(st.in(hp, (size_t)C, &d_h));
    BA_TRY(st.out(out, (size_t)C, &d_o));
    BA_TRY(ctx->scratch(SL_QUAD, (size_t)C * nvar, &quad));
    BA_TRY(laplacian_quad(ctx, *l, C, nvar, d_s, quad));
    BA_TRY(launch_laplacian_finish(ctx, C, nvar, l->P, l->logdet, quad, HpSrc{d_h, 1, nullptr}, d_o, 1));
    return st.finish();
}

// ------------------------------------------------------------------ fused FFI model
int beatamd_ffi_model_create(beatamd_ctx *ctx, const beatamd_ffi_layout *layout, int32_t nsub,
                             const int32_t *ndip, const int32_t *nstrike, const double *patch_size,
                             int32_t *model_id)
{
    ENTER(ctx);
    BA_CHECK(layout && model_id, BEATAMD_EINVAL, "ffi_model_create: bad argument");
    BA_CHECK(layout->nvar >= 0 && layout->nvar <= 3, BEATAMD_EINVAL,
             "0..3 slip variables supported, got %d", layout->nvar);
    BA_CHECK(nsub >= 0 && (nsub == 0 || (ndip && nstrike && patch_size)), BEATAMD_EINVAL,
             "ffi_model_create: subfault description missing");
    std::unique_ptr<FfiModel> m(new FfiModel());
    m->layout = *layout;
    m->nsub = nsub;
    int64_t P = 0;
    for (int s = 0; s < nsub; s++) {
        BA_CHECK(ndip[s] > 0 && nstrike[s] > 0 && patch_size[s] > 0, BEATAMD_EINVAL,
                 "subfault %d: bad discretisation", s);
        m->ndip.push_back(ndip[s]);
        m->nstrike.push_back(nstrike[s]);
        m->patch_size.push_back(patch_size[s]);
        m->patch_off.push_back((int32_t)P);
        P += (int64_t)ndip[s] * nstrike[s];
    }
    m->P = P;
    if (nsub > 0) {
        BA_TRY(m->d_ndip.alloc_copy(ctx, m->ndip.data(), (size_t)nsub));
        BA_TRY(m->d_nstrike.alloc_copy(ctx, m->nstrike.data(), (size_t)nsub));
        BA_TRY(m->d_patch_off.alloc_copy(ctx, m->patch_off.data(), (size_t)nsub));
        BA_TRY(m->d_patch_size.alloc_copy(ctx, m->patch_size.data(), (size_t)nsub));
    }
    *model_id = add_obj(ctx->models, std::move(m));
    return BEATAMD_OK;
}

// one wavemap of either domain: `data` is the observed side as the likelihood reads it, [T,N] traces or, with ntrans > 0,
// [T, hi - lo] amplitude spectra
static int add_wavemap(beatamd_ctx *ctx, int32_t model_id, const int32_t *lib_ids, const double *data, int32_t wset_id,
                       const int64_t *hp_off, const int64_t *shift_off, int32_t interpolation, int64_t ntrans, int64_t lo,
                       int64_t hi)
{
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(lib_ids && data && hp_off, BEATAMD_EINVAL, "add_wavemap: NULL argument");
    BA_CHECK(m->nsub > 0, BEATAMD_EINVAL, "add_wavemap: model has no subfaults");
    BA_CHECK(interpolation == BEATAMD_NEAREST_NEIGHBOR || interpolation == BEATAMD_MULTILINEAR,
             BEATAMD_EINVAL, "Interpolation scheme %d not implemented!", interpolation);
    Wavemap w;
    SeisLib *l0 = nullptr;
    for (int v = 0; v < m->layout.nvar; v++) {
        SeisLib *l = get_obj(ctx->seislibs, lib_ids[v]);
        BA_CHECK(l, BEATAMD_EINVAL, "add_wavemap: unknown GF library %d", lib_ids[v]);
        if (!l0) l0 = l;
        w.libs.push_back(lib_ids[v]);
    }
    BA_CHECK(l0->P == m->P, BEATAMD_EINVAL,
             "add_wavemap: library has %lld patches, fault has %lld", (long long)l0->P,
             (long long)m->P);
    w.T = l0->T;
    w.N = l0->N;
    if (ntrans > 0) {
        BA_TRY(spectrum_check_band(w.N, ntrans, lo, hi));
        const double *tw;
        BA_TRY(spectrum_twiddles(ctx, ntrans, &tw));   // (the table exists before any step can be captured)
        w.domain = BEATAMD_DOMAIN_SPECTRUM;
        w.ntrans = ntrans; w.lo = lo; w.hi = hi; w.M = hi - lo;
    }
    WeightSet *ws = get_obj(ctx->wsets, wset_id);
    BA_CHECK(ws && ws->nd == l0->T && ws->M == w.nsamples(), BEATAMD_EINVAL,
             "add_wavemap: weight set must hold %lld datasets of %lld samples%s", (long long)l0->T,
             (long long)w.nsamples(), ntrans > 0 ? " (spectrum domain: hi - lo bins)" : "");
    w.wset = wset_id;
    w.interp = interpolation;
    const int64_t np = m->layout.nparams;
    for (int64_t t = 0; t < w.T; t++) {
        BA_CHECK(hp_off[t] >= 0 && hp_off[t] < np, BEATAMD_EINVAL, "add_wavemap: hp_off[%lld] outside q",
                 (long long)t);
        if (shift_off)
            BA_CHECK(shift_off[t] >= 0 && shift_off[t] < np, BEATAMD_EINVAL,
                     "add_wavemap: shift_off[%lld] outside q", (long long)t);
    }
    if (ntrans > 0)
        BA_TRY(w.data_spec.alloc_copy(ctx, data, (size_t)w.T * w.M));
    else
        BA_TRY(w.data.alloc_copy(ctx, data, (size_t)w.T * w.N));
    BA_TRY(w.hp_off.alloc_copy(ctx, hp_off, (size_t)w.T));
    if (shift_off) {
        BA_TRY(w.shift_off.alloc_copy(ctx, shift_off, (size_t)w.T));
        // slots in the order of first appearance
        std::vector<int32_t> tslot((size_t)w.T);
        std::vector<int64_t> slot_off;
        for (int64_t t = 0; t < w.T; t++) {
            size_t k = 0;
            while (k < slot_off.size() && slot_off[k] != shift_off[t]) k++;
            if (k == slot_off.size()) slot_off.push_back(shift_off[t]);
            tslot[(size_t)t] = (int32_t)k;
        }
        if ((int64_t)slot_off.size() < w.T) {
            w.nslot = (int32_t)slot_off.size();
            BA_TRY(w.tslot.alloc_copy(ctx, tslot.data(), tslot.size()));
            BA_TRY(w.slot_shift_off.alloc_copy(ctx, slot_off.data(), slot_off.size()));
        }
    }
    m->wavemaps.push_back(std::move(w));
    return BEATAMD_OK;
}

int beatamd_ffi_model_add_wavemap(beatamd_ctx *ctx, int32_t model_id, const int32_t *lib_ids,
                                  const double *data, int32_t wset_id, const int64_t *hp_off,
                                  const int64_t *shift_off, int32_t interpolation)
{
    ENTER(ctx);
    return add_wavemap(ctx, model_id, lib_ids, data, wset_id, hp_off, shift_off, interpolation, 0, 0, 0);
}

int beatamd_ffi_model_add_wavemap_spectrum(beatamd_ctx *ctx, int32_t model_id, const int32_t *lib_ids,
                                           const double *data_spec, int32_t wset_id, const int64_t *hp_off,
                                           const int64_t *shift_off, int32_t interpolation, int64_t ntrans, int64_t lo,
                                           int64_t hi)
{
    ENTER(ctx);
    BA_CHECK(ntrans > 0, BEATAMD_EINVAL, "add_wavemap_spectrum: transform length %lld", (long long)ntrans);
    return add_wavemap(ctx, model_id, lib_ids, data_spec, wset_id, hp_off, shift_off, interpolation, ntrans, lo, hi);
}

int beatamd_amp_spectrum_batch(beatamd_ctx *ctx, int64_t R, int64_t N, int64_t ntrans, int64_t lo, int64_t hi,
                               const double *X, const double *data_spec, int64_t T, double *out)
{
    ENTER(ctx);
    BA_CHECK(X && out && R >= 0, BEATAMD_EINVAL, "amp_spectrum: bad argument");
    BA_TRY(spectrum_check_band(N, ntrans, lo, hi));
    BA_CHECK(!data_spec || T > 0, BEATAMD_EINVAL, "amp_spectrum: data_spec given with %lld datasets", (long long)T);
    if (R == 0) return BEATAMD_OK;
    const int64_t M = hi - lo;
    Staging st(ctx);
    const double *d_x, *d_d = nullptr;
    double *d_o;
    BA_TRY(st.in(X, (size_t)R * N, &d_x));
    if (data_spec) BA_TRY(st.in(data_spec, (size_t)T * M, &d_d));
    BA_TRY(st.out(out, (size_t)R * M, &d_o));
    BA_TRY(launch_amp_spectrum(ctx, R, N, N, ntrans, lo, hi, d_x, d_d, T, d_o));
    return st.finish();
}

// the datasets of a geodetic composite, checked (`fn`: the entry point, for the messages): g gets sizes, weight sets, Nobs
static int geodetic_datasets(beatamd_ctx *ctx, const FfiModel &m, const char *fn, int32_t nd, const int64_t *sizes,
                             const int32_t *wset_ids, const int64_t *hp_off, Geodetic &g)
{
    for (int d = 0; d < nd; d++) {
        BA_CHECK(sizes[d] > 0, BEATAMD_EINVAL, "%s: empty dataset %d", fn, d);
        BA_CHECK(hp_off[d] >= 0 && hp_off[d] < m.layout.nparams, BEATAMD_EINVAL, "%s: hp_off[%d] outside q", fn, d);
        WeightSet *ws = get_obj(ctx->wsets, wset_ids[d]);
        BA_CHECK(ws && ws->nd == 1 && ws->M == sizes[d], BEATAMD_EINVAL,
                 "%s: weight set of dataset %d must be 1 x %lld", fn, d, (long long)sizes[d]);
        g.sizes.push_back(sizes[d]);
        g.wsets.push_back(wset_ids[d]);
        g.Nobs += sizes[d];
    }
    return BEATAMD_OK;
}

int beatamd_ffi_model_add_geodetic(beatamd_ctx *ctx, int32_t model_id, const int32_t *geo_lib_ids,
                                   const double *data, const double *odws, int32_t nd,
                                   const int64_t *sizes, const int32_t *wset_ids,
                                   const int64_t *hp_off)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(!m->has_geo, BEATAMD_EINVAL, "model already has a geodetic composite");
    BA_CHECK(geo_lib_ids && data && odws && sizes && wset_ids && hp_off && nd > 0, BEATAMD_EINVAL,
             "add_geodetic: bad argument");
    Geodetic g;
    BA_TRY(geodetic_datasets(ctx, *m, "add_geodetic", nd, sizes, wset_ids, hp_off, g));
    int64_t P = m->P;
    for (int v = 0; v < m->layout.nvar; v++) {
        GeoLib *l = get_obj(ctx->geolibs, geo_lib_ids[v]);
        BA_CHECK(l && l->Nobs == g.Nobs, BEATAMD_EINVAL,
                 "add_geodetic: library %d missing or observation count mismatch", geo_lib_ids[v]);
        if (m->nsub > 0)
            BA_CHECK(l->P == m->P, BEATAMD_EINVAL, "add_geodetic: patch count mismatch");
        else
            P = l->P;
        g.libs.push_back(geo_lib_ids[v]);
    }
    BA_TRY(g.data.alloc_copy(ctx, data, (size_t)g.Nobs));
    BA_TRY(g.odws.alloc_copy(ctx, odws, (size_t)g.Nobs));
    BA_TRY(g.hp_off.alloc_copy(ctx, hp_off, (size_t)nd));
    m->P = P;
    m->geo = std::move(g);
    m->has_geo = true;
    m->lsq_blocks_valid = false;
    return BEATAMD_OK;
}

int beatamd_ffi_model_add_geodetic_geometry(beatamd_ctx *ctx, int32_t model_id, int32_t nsrc,
                                            const int32_t *kind, const int64_t *param_off,
                                            const double *param_fixed, int64_t nobs,
                                            const double *east, const double *north,
                                            const double *los, double nu, const double *data,
                                            const double *odws, int32_t nd, const int64_t *sizes,
                                            const int32_t *wset_ids, const int64_t *hp_off)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(!m->has_geo, BEATAMD_EINVAL, "model already has a geodetic composite");
    BA_CHECK(nsrc > 0 && kind && param_off && param_fixed && east && north && los && data && odws &&
                 sizes && wset_ids && hp_off && nd > 0 && nobs > 0,
             BEATAMD_EINVAL, "add_geodetic_geometry: bad argument");
    BA_CHECK(nu > -1.0 && nu < 0.5, BEATAMD_EINVAL, "Poisson ratio outside (-1, 0.5)");
    Geodetic g;
    BA_TRY(geodetic_datasets(ctx, *m, "add_geodetic_geometry", nd, sizes, wset_ids, hp_off, g));
    BA_CHECK(g.Nobs == nobs, BEATAMD_EINVAL, "add_geodetic_geometry: dataset sizes sum to %lld, not %lld",
             (long long)g.Nobs, (long long)nobs);
    for (int i = 0; i < nsrc * 10; i++)
        BA_CHECK(param_off[i] < m->layout.nparams, BEATAMD_EINVAL,
                 "add_geodetic_geometry: parameter offset %d outside q", i);
    for (int i = 0; i < nsrc; i++)
        BA_CHECK(kind[i] == 0 || kind[i] == 1, BEATAMD_EINVAL, "unknown source kind %d", kind[i]);
    BA_TRY(g.data.alloc_copy(ctx, data, (size_t)nobs));
    BA_TRY(g.odws.alloc_copy(ctx, odws, (size_t)nobs));
    BA_TRY(g.hp_off.alloc_copy(ctx, hp_off, (size_t)nd));
    GeomSources gs;
    gs.nsrc = nsrc;
    gs.Nobs = nobs;
    gs.nu = nu;
    BA_TRY(gs.kind.alloc_copy(ctx, kind, (size_t)nsrc));
    BA_TRY(gs.poff.alloc_copy(ctx, param_off, (size_t)nsrc * 10));
    BA_TRY(gs.pfix.alloc_copy(ctx, param_fixed, (size_t)nsrc * 10));
    BA_TRY(gs.east.alloc_copy(ctx, east, (size_t)nobs));
    BA_TRY(gs.north.alloc_copy(ctx, north, (size_t)nobs));
    BA_TRY(gs.los.alloc_copy(ctx, los, (size_t)nobs * 3));
    m->geom = std::move(gs);
    m->geo = std::move(g);
    m->has_geo = true;
    m->geo_is_geometry = true;
    return BEATAMD_OK;
}

// ------------------------------------------------------------------ polarity composite (polarity.hip)
// the source of a polarity call from its host tables: kind, offsets in [-1, nparams), the variables of the kind
static int pol_source_arg(beatamd_ctx *ctx, int32_t kind, const int64_t *param_off, const double *param_fixed, int64_t nparams,
                          PolSource *s, const char *who)
{
    BA_CHECK(kind == POL_MTQT || kind == POL_MT || kind == POL_DC, BEATAMD_EINVAL, "%s: unknown source kind %d", who, kind);
    BA_CHECK(param_off && param_fixed, BEATAMD_EINVAL, "%s: NULL source table", who);
    std::vector<int64_t> off;
    std::vector<double> fix;
    BA_TRY(host_copy(ctx, param_off, 6, off));
    BA_TRY(host_copy(ctx, param_fixed, 6, fix));
    s->kind = kind;
    const int nv = kind == POL_MTQT ? 5 : (kind == POL_MT ? 6 : 3);
    for (int k = 0; k < 6; k++) {
        BA_CHECK(off[k] >= -1 && off[k] < nparams, BEATAMD_EINVAL, "%s: offset %lld of source variable %d outside q", who,
                 (long long)off[k], k);
        s->off[k] = k < nv ? off[k] : -1;
        s->fix[k] = k < nv ? fix[k] : 0.0;
    }
    return BEATAMD_OK;
}

// U_MAPPING must be strictly increasing for numpy.interp's search to be defined
static int pol_tables_arg(beatamd_ctx *ctx, int32_t kind, int64_t ntab, const double *utab, const double *btab, const char *who)
{
    if (kind != POL_MTQT) return BEATAMD_OK;
    BA_CHECK(ntab >= 2 && ntab <= 1000000 && utab && btab, BEATAMD_EINVAL, "%s: the mtqt source needs the w -> beta tables", who);
    std::vector<double> u;
    BA_TRY(host_copy(ctx, utab, (size_t)ntab, u));
    for (int64_t i = 1; i < ntab; i++)
        BA_CHECK(u[i] > u[i - 1], BEATAMD_EINVAL, "%s: the u table is not strictly increasing at %lld", who, (long long)i);
    return BEATAMD_OK;
}

int beatamd_ffi_model_add_polarity(beatamd_ctx *ctx, int32_t model_id, int32_t kind, const int64_t *param_off,
                                   const double *param_fixed, int32_t nmap, const int64_t *n_t, const double *rw,
                                   const double *obs, double gamma, const int64_t *hp_off, const double *hp_fixed, int64_t ntab,
                                   const double *utab, const double *btab)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(!m->has_pol, BEATAMD_EINVAL, "model already has a polarity composite");
    BA_CHECK(nmap >= 1 && nmap <= POL_MAX_MAPS && n_t && rw && obs && hp_off && hp_fixed, BEATAMD_EINVAL,
             "add_polarity: bad argument (1 to %d polarity maps)", POL_MAX_MAPS);
    BA_CHECK(gamma >= 0.0 && gamma <= 0.5, BEATAMD_EINVAL, "add_polarity: gamma %g outside [0, 0.5]", gamma);
    const int64_t np = m->layout.nparams;
    Polarity p;
    BA_TRY(pol_source_arg(ctx, kind, param_off, param_fixed, np, &p.src, "add_polarity"));
    BA_TRY(pol_tables_arg(ctx, kind, ntab, utab, btab, "add_polarity"));
    std::vector<int64_t> nt, ho;
    std::vector<double> hf;
    BA_TRY(host_copy(ctx, n_t, (size_t)nmap, nt));
    BA_TRY(host_copy(ctx, hp_off, (size_t)nmap, ho));
    BA_TRY(host_copy(ctx, hp_fixed, (size_t)nmap, hf));
    p.nmap = nmap;
    p.gamma = gamma;
    for (int i = 0; i < nmap; i++) {
        BA_CHECK(nt[i] >= 1, BEATAMD_EINVAL, "add_polarity: map %d has no station", i);
        BA_CHECK(ho[i] >= -1 && ho[i] < np, BEATAMD_EINVAL, "add_polarity: hyper-parameter offset of map %d outside q", i);
        p.NT += nt[i];
        p.map_end[i] = p.NT;
        p.hp_off[i] = ho[i];
        p.hp_fix[i] = hf[i];
    }
    for (int i = nmap; i < POL_MAX_MAPS; i++) {
        p.map_end[i] = p.NT;
        p.hp_off[i] = -1;
    }
    BA_CHECK(p.NT < (int64_t)0x7fffffff, BEATAMD_EINVAL, "add_polarity: too many stations");
    BA_TRY(p.rw.alloc_copy(ctx, rw, (size_t)p.NT * 6));
    BA_TRY(p.obs.alloc_copy(ctx, obs, (size_t)p.NT));
    if (kind == POL_MTQT) {
        p.ntab = (int32_t)ntab;
        BA_TRY(p.utab.alloc_copy(ctx, utab, (size_t)ntab));
        BA_TRY(p.btab.alloc_copy(ctx, btab, (size_t)ntab));
    }
    m->pol = std::move(p);
    m->has_pol = true;
    return BEATAMD_OK;
}

// m6 (out [C, 6]) or the amplitudes at NT stations (rw given: out [C, NT]) of a population, by k_polarity
static int pol_population(beatamd_ctx *ctx, const char *who, int32_t kind, int64_t C, int64_t nparams, const double *Q,
                          const int64_t *param_off, const double *param_fixed, int64_t ntab, const double *utab,
                          const double *btab, int64_t NT, const double *rw, double *out)
{
    BA_CHECK(C >= 0 && nparams > 0 && Q && out && (!rw || NT >= 1), BEATAMD_EINVAL, "%s: bad argument", who);
    PolArgs a;
    BA_TRY(pol_source_arg(ctx, kind, param_off, param_fixed, nparams, &a.src, who));
    BA_TRY(pol_tables_arg(ctx, kind, ntab, utab, btab, who));
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    BA_TRY(st.in(Q, (size_t)C * nparams, &a.Q));
    if (kind == POL_MTQT) {
        BA_TRY(st.in(utab, (size_t)ntab, &a.utab));
        BA_TRY(st.in(btab, (size_t)ntab, &a.btab));
        a.ntab = (int32_t)ntab;
    }
    if (rw) BA_TRY(st.in(rw, (size_t)NT * 6, &a.rw));
    a.mode = rw ? POL_OUT_AMP : POL_OUT_M6;
    a.NT = rw ? NT : 0;
    a.ld = rw ? NT : 6;
    a.nparams = nparams;
    a.C = C;
    BA_TRY(st.out(out, (size_t)C * a.ld, &a.out));
    BA_TRY(launch_polarity(ctx, a));
    return st.finish();
}

int beatamd_mt6_batch(beatamd_ctx *ctx, int32_t kind, int64_t C, int64_t nparams, const double *Q, const int64_t *param_off,
                      const double *param_fixed, int64_t ntab, const double *utab, const double *btab, double *m6)
{
    ENTER(ctx);
    return pol_population(ctx, "mt6_batch", kind, C, nparams, Q, param_off, param_fixed, ntab, utab, btab, 0, nullptr, m6);
}

int beatamd_polarity_amplitudes_batch(beatamd_ctx *ctx, int32_t kind, int64_t C, int64_t nparams, const double *Q,
                                      const int64_t *param_off, const double *param_fixed, int64_t ntab, const double *utab,
                                      const double *btab, int64_t NT, const double *rw, double *amplitudes)
{
    ENTER(ctx);
    BA_CHECK(rw, BEATAMD_EINVAL, "polarity_amplitudes_batch: no radiation weights");
    return pol_population(ctx, "polarity_amplitudes_batch", kind, C, nparams, Q, param_off, param_fixed, ntab, utab, btab, NT,
                          rw, amplitudes);
}

int beatamd_w_to_beta_batch(beatamd_ctx *ctx, int64_t n, const double *w, int64_t ntab, const double *utab, const double *btab,
                            double *beta)
{
    ENTER(ctx);
    BA_CHECK(n >= 0 && w && beta, BEATAMD_EINVAL, "w_to_beta_batch: bad argument");
    BA_TRY(pol_tables_arg(ctx, POL_MTQT, ntab, utab, btab, "w_to_beta_batch"));
    if (n == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_w, *d_u, *d_b;
    double *d_o;
    BA_TRY(st.in(w, (size_t)n, &d_w));
    BA_TRY(st.in(utab, (size_t)ntab, &d_u));
    BA_TRY(st.in(btab, (size_t)ntab, &d_b));
    BA_TRY(st.out(beta, (size_t)n, &d_o));
    BA_TRY(launch_w_to_beta(ctx, n, d_w, d_u, d_b, (int)ntab, d_o));
    return st.finish();
}

int beatamd_ffi_model_add_geodetic_corrections(beatamd_ctx *ctx, int32_t model_id, int32_t nterm,
                                               const int32_t *dataset, const int32_t *ncol,
                                               const double *basis, const int64_t *coef_off,
                                               const double *coef_fixed)
{
    // every kind 0
    return beatamd_ffi_model_add_geodetic_corrections_kinds(ctx, model_id, nterm, dataset, ncol, basis, coef_off, coef_fixed,
                                                            nullptr, nullptr);
}

int beatamd_ffi_model_add_geodetic_corrections_kinds(beatamd_ctx *ctx, int32_t model_id, int32_t nterm,
                                                     const int32_t *dataset, const int32_t *ncol,
                                                     const double *basis, const int64_t *coef_off,
                                                     const double *coef_fixed, const int32_t *kind,
                                                     const double *earth)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(m->has_geo, BEATAMD_EINVAL, "add_geodetic_corrections: the model has no geodetic composite");
    Geodetic &g = m->geo;
    BA_CHECK(!g.corr_set, BEATAMD_EINVAL, "add_geodetic_corrections: the composite already has its corrections");
    BA_CHECK(nterm >= 0 && nterm <= GEO_CORR_MAX, BEATAMD_EINVAL,
             "add_geodetic_corrections: %d terms, the table holds %d", nterm, GEO_CORR_MAX);
    BA_CHECK(nterm == 0 || (dataset && ncol && basis && coef_off && coef_fixed), BEATAMD_EINVAL,
             "add_geodetic_corrections: bad argument");
    m->obs_quads_valid = false;
    m->lsq_blocks_valid = false;
    if (nterm == 0) {
        g.corr_set = true;
        return BEATAMD_OK;
    }
    std::vector<int32_t> ds, nc;
    std::vector<int64_t> off;
    std::vector<double> fix;
    BA_TRY(host_copy(ctx, dataset, (size_t)nterm, ds));
    BA_TRY(host_copy(ctx, ncol, (size_t)nterm, nc));
    BA_TRY(host_copy(ctx, coef_off, (size_t)nterm * 4, off));
    BA_TRY(host_copy(ctx, coef_fixed, (size_t)nterm * 4, fix));
    std::vector<int32_t> kd((size_t)nterm, GEO_CORR_LINEAR);
    std::vector<double> ea((size_t)nterm * 3, 0.0);
    BA_CHECK((kind == nullptr) == (earth == nullptr), BEATAMD_EINVAL,
             "add_geodetic_corrections: kind and earth come together");
    if (kind) {
        BA_TRY(host_copy(ctx, kind, (size_t)nterm, kd));
        BA_TRY(host_copy(ctx, earth, (size_t)nterm * 3, ea));
    }
    std::vector<PoleTerm> poles;
    const int nd = (int)g.sizes.size();
    std::vector<int64_t> start((size_t)nd, 0);
    for (int d = 1; d < nd; d++) start[d] = start[d - 1] + g.sizes[d - 1];
    std::vector<GeoCorrTerm> terms((size_t)nterm);
    int64_t nbasis = 0;
    for (int j = 0; j < nterm; j++) {
        BA_CHECK(ds[j] >= 0 && ds[j] < nd, BEATAMD_EINVAL,
                 "add_geodetic_corrections: term %d names dataset %d of %d", j, ds[j], nd);
        BA_CHECK(j == 0 || ds[j] >= ds[j - 1], BEATAMD_EINVAL,
                 "add_geodetic_corrections: the dataset indices decrease at term %d", j);
        BA_CHECK(nc[j] >= 1 && nc[j] <= 4, BEATAMD_EINVAL,
                 "add_geodetic_corrections: term %d has %d basis columns (1..4)", j, nc[j]);
        GeoCorrTerm &t = terms[(size_t)j];
        memset(&t, 0, sizeof(t));
        t.start = start[ds[j]];
        t.n = g.sizes[ds[j]];
        t.K = nc[j];
        for (int k = 0; k < 4; k++) {
            const int64_t o = k < nc[j] ? off[(size_t)j * 4 + k] : -1;
            BA_CHECK(o >= -1 && o < m->layout.nparams, BEATAMD_EINVAL,
                     "add_geodetic_corrections: coefficient %d of term %d: offset %lld outside q", k, j, (long long)o);
            t.off[k] = o;
            t.fix[k] = k < nc[j] ? fix[(size_t)j * 4 + k] : 0.0;
        }
        BA_CHECK(kd[j] == GEO_CORR_LINEAR || kd[j] == GEO_CORR_POLE, BEATAMD_EINVAL,
                 "add_geodetic_corrections: term %d has the unknown kind %d", j, kd[j]);
        t.kind = kd[j];
        if (kd[j] == GEO_CORR_POLE) {
            BA_CHECK(nc[j] == 3, BEATAMD_EINVAL,
                     "add_geodetic_corrections: the Euler-pole term %d has %d basis columns, not 3", j, nc[j]);
            const double *e = &ea[(size_t)j * 3];
            BA_CHECK(e[0] > 0.0 && e[1] > 0.0 && e[2] >= 0.0 && e[2] < 1.0, BEATAMD_EINVAL,
                     "add_geodetic_corrections: term %d: earth (radius %g, equator radius %g, oblateness %g)", j, e[0], e[1], e[2]);
            PoleTerm pt;
            for (int k = 0; k < 3; k++) { pt.off[k] = t.off[k]; pt.fix[k] = t.fix[k]; pt.earth[k] = e[k]; }
            t.rec = (int32_t)poles.size();
            poles.push_back(pt);
        }
        nbasis += t.n * t.K;
    }
    DevMem<double> d_basis;
    BA_TRY(d_basis.alloc_copy(ctx, basis, (size_t)nbasis));
    int64_t bo = 0;
    for (int j = 0; j < nterm; j++) {
        terms[(size_t)j].B = d_basis.get() + bo;
        bo += terms[(size_t)j].n * terms[(size_t)j].K;
    }
    DevMem<GeoCorrTerm> d_terms;
    BA_TRY(d_terms.alloc_copy(ctx, terms.data(), terms.size()));
    // the pole terms' inputs and one chain's worth of records (the chains' come with the first evaluation,
    // geo_pole_coefficients): everything that can fail is allocated before anything is installed
    DevMem<PoleTerm> d_poles;
    DevMem<double> d_rec;
    if (!poles.empty()) {
        BA_TRY(d_poles.alloc_copy(ctx, poles.data(), poles.size()));
        BA_TRY(d_rec.alloc(poles.size() * 4));
    }
    g.corr_basis = std::move(d_basis);
    g.corr_terms = std::move(d_terms);
    g.corr.terms = g.corr_terms.get();
    g.corr.nterm = nterm;
    if (!poles.empty()) {
        g.pole_terms = std::move(d_poles);
        g.pole_coef = std::move(d_rec);
        g.pole_chains = 1;
        g.corr.npole = (int32_t)poles.size();
        g.corr.pole_terms = g.pole_terms.get();
        g.corr.pole_stride = (int64_t)poles.size() * 4;
        g.corr.pole = g.pole_coef.get();
    }
    g.corr_set = true;
    return BEATAMD_OK;
}

int beatamd_ffi_model_set_laplacian(beatamd_ctx *ctx, int32_t model_id, int32_t lap_id)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    Laplacian *l;
    BA_TRY(find_lap(ctx, lap_id, &l));
    BA_CHECK(m->layout.h_laplacian_off >= 0 && m->layout.h_laplacian_off < m->layout.nparams,
             BEATAMD_EINVAL, "set_laplacian: layout has no h_laplacian offset");
    BA_CHECK(m->P == 0 || l->P == m->P, BEATAMD_EINVAL, "set_laplacian: patch count mismatch");
    if (m->P == 0) m->P = l->P;
    m->lap = lap_id;
    m->lsq_blocks_valid = false;
    return BEATAMD_OK;
}

int beatamd_ffi_model_nllk(beatamd_ctx *ctx, int32_t model_id, int64_t *nllk)
{
    BA_CHECK(ctx && nllk, BEATAMD_EINVAL, "bad argument");
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    *nllk = m->nllk();
    return BEATAMD_OK;
}

int beatamd_ffi_model_destroy(beatamd_ctx *ctx, int32_t model_id)
{
    ENTER(ctx);
    return destroy_obj(ctx, ctx->models, model_id, "model");
}

int beatamd_ffi_synthetics_batch(beatamd_ctx *ctx, int32_t model_id, int32_t wavemap_index, int64_t C,
                                 const double *Q, int32_t residuals, double *out)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(Q && out && C >= 0, BEATAMD_EINVAL, "ffi_synthetics: bad argument");
    BA_CHECK(wavemap_index >= 0 && (size_t)wavemap_index < m->wavemaps.size(), BEATAMD_EINVAL,
             "ffi_synthetics: model has no wavemap %d", wavemap_index);
    BA_TRY(model_check_layout(*m));
    if (C == 0) return BEATAMD_OK;
    Wavemap &wm = m->wavemaps[wavemap_index];
    Staging st(ctx);
    const double *d_q;
    double *d_o, *st0;
    int32_t *chain_bad;
    BA_TRY(st.in(Q, (size_t)C * m->layout.nparams, &d_q));
    BA_TRY(st.out(out, (size_t)C * wm.T * wm.nsamples(), &d_o));
    BA_TRY(model_start_times(ctx, *m, C, d_q, &st0, &chain_bad));
    GfStackCall k;
    BA_TRY(wavemap_call(ctx, *m, wm, C, d_q, st0, chain_bad, &k));
    // Where this entry differs from the likelihood's call of the same wavemap, kept as found: index tables per target
    // although targets share shift variables, the float64 rows although the wavemap is set to float copies, every chain
    k.st.nslot = 0; k.st.tslot = nullptr; k.st.slot_shift_off = nullptr;
    k.f32 = false; k.active = nullptr;
    if (wm.domain == BEATAMD_DOMAIN_SPECTRUM) {
        // the time-domain stack into scratch, its amplitude spectra (or data_spec - them, seismic.py:932-941) out
        k.mode = GF_STORE_SYN;
        BA_TRY(ctx->scratch(SL_RESID, (size_t)C * wm.T * wm.N, &k.out));
        BA_TRY(launch_gfstack(ctx, k));
        BA_TRY(launch_amp_spectrum(ctx, C * wm.T, wm.N, wm.N, wm.ntrans, wm.lo, wm.hi, k.out,
                                   residuals ? wm.data_spec.get() : nullptr, wm.T, d_o));
        BA_TRY(ctx->check_status());
        return st.finish();
    }
    k.mode = residuals ? GF_RESID_STORE : GF_STORE_SYN;
    k.out = d_o;
    BA_TRY(launch_gfstack(ctx, k));
    BA_TRY(ctx->check_status());   // an index outside the library is the reference's IndexError
    return st.finish();
}

int beatamd_ffi_start_times_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, double *times,
                                  int32_t *chain_bad)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(Q && times && C >= 0, BEATAMD_EINVAL, "ffi_start_times: bad argument");
    BA_TRY(model_check_layout(*m));
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_q;
    double *d_t, *st0;
    int32_t *d_b = nullptr, *bad;
    BA_TRY(st.in(Q, (size_t)C * m->layout.nparams, &d_q));
    BA_TRY(st.out(times, (size_t)C * m->P, &d_t));
    if (chain_bad) BA_TRY(st.out(chain_bad, (size_t)C, &d_b));
    BA_TRY(model_start_times(ctx, *m, C, d_q, &st0, &bad));
    BA_HIP(hipMemcpyAsync(d_t, st0, (size_t)C * m->P * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if (d_b) BA_HIP(hipMemcpyAsync(d_b, bad, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    BA_TRY(st.finish());            // (host arrays are filled before a raised status word is returned)
    return ctx->check_status();     // a hypocentre outside the patch grid: the flags say which chains
}

// ---- moment, magnitude and moment-rate functions of a batch of draws (momentrate.hip)
namespace {

// the slip components of a moment: comp_off [ncomp] offsets in q (host or device array), or NULL: the layout's own
int mr_components(beatamd_ctx *ctx, const FfiModel &m, const int64_t *comp_off, int32_t ncomp, const char *what, MrComps *out)
{
    const beatamd_ffi_layout &L = m.layout;
    if (!comp_off) {
        out->n = L.nvar;
        for (int v = 0; v < L.nvar; v++) out->off[v] = L.slip_off[v];
    } else {
        BA_CHECK(ncomp >= 1 && ncomp <= 4, BEATAMD_EINVAL, "%s: %d slip components (1 ... 4)", what, ncomp);
        std::vector<int64_t> off;
        BA_TRY(host_copy(ctx, comp_off, (size_t)ncomp, off));
        out->n = ncomp;
        for (int v = 0; v < ncomp; v++) out->off[v] = off[(size_t)v];
    }
    BA_CHECK(out->n >= 1 && out->n <= 4, BEATAMD_EINVAL, "%s: the model has no slip variable", what);
    for (int v = 0; v < out->n; v++)
        BA_CHECK(out->off[v] >= 0 && out->off[v] + m.P <= L.nparams, BEATAMD_EINVAL, "%s: slip component %d outside q", what, v);
    return BEATAMD_OK;
}

// the onsets of the batch: the caller's (start_times [C,P], chain_bad [C] nullable) or the model's sweep
int mr_start_times(beatamd_ctx *ctx, const FfiModel &m, Staging &st, int64_t C, const double *d_q, const double *start_times,
                   const int32_t *chain_bad, const char *what, const double **st0, const int32_t **bad)
{
    const beatamd_ffi_layout &L = m.layout;
    BA_CHECK(m.nsub >= 1 && m.P >= 1, BEATAMD_EINVAL, "%s: the model has no subfault", what);
    BA_CHECK(L.durations_off >= 0 && L.durations_off + m.P <= L.nparams, BEATAMD_EINVAL, "%s: layout: durations outside q", what);
    if (start_times) {
        BA_TRY(st.in(start_times, (size_t)C * m.P, st0));
        *bad = nullptr;
        if (chain_bad) BA_TRY(st.in(chain_bad, (size_t)C, bad));
        return BEATAMD_OK;
    }
    BA_CHECK(!chain_bad, BEATAMD_EINVAL, "%s: chain_bad without start_times", what);
    BA_CHECK(L.velocities_off >= 0 && L.velocities_off + m.P <= L.nparams && L.nuc_strike_off >= 0 &&
                 L.nuc_strike_off + m.nsub <= L.nparams && L.nuc_dip_off >= 0 && L.nuc_dip_off + m.nsub <= L.nparams &&
                 L.time_off >= 0 && L.time_off + m.nsub <= L.nparams,
             BEATAMD_EINVAL, "%s: layout: rupture variables outside q", what);
    double *t;
    int32_t *b;
    BA_TRY(model_start_times(ctx, m, C, d_q, &t, &b));
    *st0 = t;
    *bad = b;
    return BEATAMD_OK;
}

}  // namespace

int beatamd_ffi_magnitudes_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, const double *moment_per_slip,
                                 const int64_t *comp_off, int32_t ncomp, double *M0, double *Mw)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(Q && moment_per_slip && M0 && Mw && C >= 0, BEATAMD_EINVAL, "ffi_magnitudes: bad argument");
    BA_CHECK(m->P >= 1 && m->layout.nparams > 0, BEATAMD_EINVAL, "ffi_magnitudes: the model has no patches");
    MrComps comps;
    BA_TRY(mr_components(ctx, *m, comp_off, ncomp, "ffi_magnitudes", &comps));
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_q, *d_k;
    double *d_m0, *d_mw;
    BA_TRY(st.in(Q, (size_t)C * m->layout.nparams, &d_q));
    BA_TRY(st.in(moment_per_slip, (size_t)m->P, &d_k));
    BA_TRY(st.out(M0, (size_t)C, &d_m0));
    BA_TRY(st.out(Mw, (size_t)C, &d_mw));
    BA_TRY(launch_moment_magnitude(ctx, C, m->P, d_q, m->layout.nparams, comps, d_k, d_m0, d_mw));
    return st.finish();
}

int beatamd_ffi_moment_rate_spans_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q,
                                        const double *start_times, const int32_t *chain_bad, double deltat, int64_t *spans)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(Q && spans && C >= 0, BEATAMD_EINVAL, "ffi_moment_rate_spans: bad argument");
    BA_CHECK(deltat > 0.0 && deltat <= 1.79769313486231570815e+308, BEATAMD_EINVAL, "ffi_moment_rate_spans: deltat %g", deltat);
    BA_CHECK(m->layout.nparams > 0, BEATAMD_EINVAL, "ffi_moment_rate_spans: layout: nparams must be positive");
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_q, *st0;
    const int32_t *bad;
    int64_t *d_s;
    BA_TRY(st.in(Q, (size_t)C * m->layout.nparams, &d_q));
    BA_TRY(mr_start_times(ctx, *m, st, C, d_q, start_times, chain_bad, "ffi_moment_rate_spans", &st0, &bad));
    BA_TRY(st.out(spans, (size_t)C * (m->nsub + 1) * 2, &d_s));
    BA_TRY(launch_moment_rate_span(ctx, *m, C, d_q, st0, bad, deltat, d_s));
    BA_TRY(st.finish());            // (host arrays are filled before a raised status word is returned)
    return ctx->check_status();     // a hypocentre outside the patch grid, an onset that is not finite
}

int beatamd_ffi_moment_rates_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, const double *moment_per_slip,
                                   const int64_t *comp_off, int32_t ncomp, const double *start_times, const int32_t *chain_bad,
                                   double deltat, int32_t stf, int64_t kbase, int64_t NT, double *rates, int64_t *spans)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(Q && moment_per_slip && rates && C >= 0, BEATAMD_EINVAL, "ffi_moment_rates: bad argument");
    BA_CHECK(stf == BEATAMD_STF_HALF_SINUSOID, BEATAMD_EINVAL,
             "ffi_moment_rates: source-time function %d (only BEATAMD_STF_HALF_SINUSOID = 0 is built)", stf);
    BA_CHECK(deltat > 0.0 && deltat <= 1.79769313486231570815e+308, BEATAMD_EINVAL, "ffi_moment_rates: deltat %g", deltat);
    BA_CHECK(NT >= 1 && NT <= MR_NT_MAX, BEATAMD_EINVAL, "ffi_moment_rates: %lld samples per row (1 ... %d: the row lives in LDS)",
             (long long)NT, MR_NT_MAX);
    BA_CHECK(kbase >= -((int64_t)1 << 41) && kbase <= ((int64_t)1 << 41), BEATAMD_EINVAL, "ffi_moment_rates: kbase %lld",
             (long long)kbase);
    BA_CHECK(m->layout.nparams > 0, BEATAMD_EINVAL, "ffi_moment_rates: layout: nparams must be positive");
    MrComps comps;
    BA_TRY(mr_components(ctx, *m, comp_off, ncomp, "ffi_moment_rates", &comps));
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_q, *d_k, *st0;
    const int32_t *bad;
    double *d_r;
    int64_t *d_s;
    BA_TRY(st.in(Q, (size_t)C * m->layout.nparams, &d_q));
    BA_TRY(st.in(moment_per_slip, (size_t)m->P, &d_k));
    BA_TRY(mr_start_times(ctx, *m, st, C, d_q, start_times, chain_bad, "ffi_moment_rates", &st0, &bad));
    BA_TRY(st.out(rates, (size_t)C * (m->nsub + 1) * NT, &d_r));
    if (spans) BA_TRY(st.out(spans, (size_t)C * (m->nsub + 1) * 2, &d_s));
    else BA_TRY(ctx->scratch(SL_MR_SPANS, (size_t)C * (m->nsub + 1) * 2, &d_s));
    BA_TRY(launch_moment_rate_span(ctx, *m, C, d_q, st0, bad, deltat, d_s));
    BA_TRY(launch_moment_rate(ctx, *m, C, d_q, st0, comps, d_k, deltat, d_s, kbase, NT, d_r));
    BA_TRY(st.finish());
    return ctx->check_status();     // flagged draws and draws outside the grid have NaN rows
}

int beatamd_ffi_logp_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, double *LL)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(Q && LL && C >= 0, BEATAMD_EINVAL, "ffi_logp: bad argument");
    BA_TRY(model_check_layout(*m));
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_q;
    double *d_l;
    BA_TRY(st.in(Q, (size_t)C * m->layout.nparams, &d_q));
    BA_TRY(st.out(LL, (size_t)C * m->nllk(), &d_l));
    BA_TRY(ffi_logp_device(ctx, *m, C, d_q, d_l));
    return st.finish();
}

int beatamd_ffi_model_nterm(beatamd_ctx *ctx, int32_t model_id, int64_t *nterm)
{
    BA_CHECK(ctx && nterm, BEATAMD_EINVAL, "bad argument");
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    *nterm = model_nterm(*m);
    return BEATAMD_OK;
}

int beatamd_ffi_llks_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, double *llks)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(Q && llks && C >= 0, BEATAMD_EINVAL, "ffi_llks: bad argument");
    BA_TRY(model_check_layout(*m));
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_q;
    double *d_l;
    BA_TRY(st.in(Q, (size_t)C * m->layout.nparams, &d_q));
    BA_TRY(st.out(llks, (size_t)C * model_nterm(*m), &d_l));
    LogpOpts opt;
    opt.llks = d_l;
    BA_TRY(ffi_logp_device(ctx, *m, C, d_q, nullptr, opt));
    return st.finish();
}

// ------------------------------------------------------------------ lsq start (lsq.hip)
int beatamd_ffi_model_set_lsq_variables(beatamd_ctx *ctx, int32_t model_id, int32_t inverted, int32_t zeroed)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(inverted >= 0 && inverted < m->layout.nvar && zeroed >= -1 && zeroed < m->layout.nvar && zeroed != inverted,
             BEATAMD_EINVAL, "set_lsq_variables: slip variables %d / %d of %d", inverted, zeroed, m->layout.nvar);
    if (m->lsq_var != inverted) m->lsq_blocks_valid = false;
    m->lsq_var = inverted;
    m->lsq_zero_var = zeroed;
    return BEATAMD_OK;
}

// BEATAMD_NNLS_MAXITER (tests): the iteration cap instead of 3 n
static int nnls_maxiter()
{
    const char *e = getenv("BEATAMD_NNLS_MAXITER");
    return e && *e ? atoi(e) : 0;
}

int beatamd_ffi_lsq_normal_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, double *N, double *b,
                                 int32_t *chain_bad)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(Q && N && b && C >= 0, BEATAMD_EINVAL, "ffi_lsq_normal: bad argument");
    BA_TRY(model_check_layout(*m));
    if (C == 0) return BEATAMD_OK;
    const int64_t P = m->P;
    Staging st(ctx);
    const double *d_q;
    double *d_n, *d_b;
    int32_t *d_bad = nullptr, *bad = nullptr;
    BA_TRY(st.in(Q, (size_t)C * m->layout.nparams, &d_q));
    BA_TRY(st.out(N, (size_t)(C * P * P), &d_n));
    BA_TRY(st.out(b, (size_t)(C * P), &d_b));
    if (chain_bad) BA_TRY(st.out(chain_bad, (size_t)C, &d_bad));
    BA_TRY(lsq_normal_device(ctx, *m, C, d_q, d_n, d_b, &bad));
    if (d_bad) {
        if (bad) BA_HIP(hipMemcpyAsync(d_bad, bad, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
        else BA_HIP(hipMemsetAsync(d_bad, 0, (size_t)C * sizeof(int32_t), ctx->stream));
    }
    BA_TRY(st.finish());            // (host arrays are filled before a raised status word is returned)
    return ctx->check_status();     // a time outside the library grid: the flags say which chains
}

int beatamd_nnls_batch(beatamd_ctx *ctx, int64_t C, int64_t n, const double *N, const double *b, double *x, int32_t *iters,
                       int32_t *status)
{
    ENTER(ctx);
    BA_CHECK(N && b && x && iters && status && C >= 0 && n >= 1, BEATAMD_EINVAL, "nnls: bad argument");
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_n, *d_b;
    double *d_x;
    int32_t *d_it, *d_st;
    BA_TRY(st.in(N, (size_t)(C * n * n), &d_n));
    BA_TRY(st.in(b, (size_t)(C * n), &d_b));
    BA_TRY(st.out(x, (size_t)(C * n), &d_x));
    BA_TRY(st.out(iters, (size_t)C, &d_it));
    BA_TRY(st.out(status, (size_t)C, &d_st));
    BA_TRY(launch_nnls(ctx, C, n, d_n, d_b, d_x, d_it, d_st, nnls_maxiter()));
    return st.finish();
}

int beatamd_ffi_lsq_solution_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q_in, double *Q_out,
                                   int32_t *iters, int32_t *status)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(Q_in && Q_out && iters && status && C >= 0, BEATAMD_EINVAL, "ffi_lsq_solution: bad argument");
    BA_TRY(model_check_layout(*m));
    if (C == 0) return BEATAMD_OK;
    const int64_t P = m->P, np = m->layout.nparams;
    BA_CHECK(m->lsq_var >= 0, BEATAMD_EINVAL,
             "lsq: the model has no inverted slip variable (beatamd_ffi_model_set_lsq_variables)");
    Staging st(ctx);
    const double *d_qi;
    double *d_qo;
    int32_t *d_it, *d_st;
    BA_TRY(st.in(Q_in, (size_t)C * np, &d_qi));
    BA_TRY(st.out(Q_out, (size_t)C * np, &d_qo));
    BA_TRY(st.out(iters, (size_t)C, &d_it));
    BA_TRY(st.out(status, (size_t)C, &d_st));
    // chains per pass: the normal matrices of a pass stay within 1 GiB of scratch
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(C, ((int64_t)1 << 30) / std::max<int64_t>(1, P * P * 8)));
    const int maxiter = nnls_maxiter();
    for (int64_t c0 = 0; c0 < C; c0 += chunk) {
        const int64_t cc = std::min(chunk, C - c0);
        double *nm, *bv, *x;
        int32_t *bad;
        BA_TRY(ctx->scratch(SL_LSQ_N, (size_t)(cc * P * P), &nm));
        BA_TRY(ctx->scratch(SL_LSQ_B, (size_t)(cc * P), &bv));
        BA_TRY(ctx->scratch(SL_LSQ_X, (size_t)(cc * P), &x));
        BA_TRY(lsq_normal_device(ctx, *m, cc, d_qi + c0 * np, nm, bv, &bad));
        BA_TRY(launch_nnls(ctx, cc, P, nm, bv, x, d_it + c0, d_st + c0, maxiter));
        if (d_qo != d_qi)
            BA_HIP(hipMemcpyAsync(d_qo + c0 * np, d_qi + c0 * np, (size_t)(cc * np) * sizeof(double), hipMemcpyDeviceToDevice,
                                  ctx->stream));
        BA_TRY(launch_lsq_scatter(ctx, cc, P, x, d_qo + c0 * np, np, m->layout.slip_off[m->lsq_var],
                                  m->lsq_zero_var >= 0 ? m->layout.slip_off[m->lsq_zero_var] : -1));
    }
    BA_TRY(st.finish());
    return ctx->check_status();     // a time outside the library grid is the reference's IndexError
}

// ------------------------------------------------------------------ posterior diagnostics (summary.hip)
int beatamd_wset_quad_batch(beatamd_ctx *ctx, int32_t wset_id, int64_t C, const double *R, double *quad)
{
    ENTER(ctx);
    WeightSet *w;
    BA_TRY(find_wset(ctx, wset_id, &w));
    BA_CHECK(R && quad && C >= 0, BEATAMD_EINVAL, "wset_quad: bad argument");
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_r;
    double *d_q;
    BA_TRY(st.in(R, (size_t)C * w->nd * w->M, &d_r));
    BA_TRY(st.out(quad, (size_t)C * w->nd, &d_q));
    BA_TRY(wset_quad(ctx, *w, C, d_r, w->nd * w->M, w->M, d_q));
    return st.finish();
}

int beatamd_ffi_obs_quads(beatamd_ctx *ctx, int32_t model_id, double *denom)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(denom, BEATAMD_EINVAL, "ffi_obs_quads: bad argument");
    BA_TRY(model_check_layout(*m));
    BA_TRY(model_obs_quads(ctx, *m));
    const int64_t ndata = model_ndata(*m);
    if (ndata == 0) return BEATAMD_OK;
    Staging st(ctx);
    double *d_o;
    BA_TRY(st.out(denom, (size_t)ndata, &d_o));
    BA_HIP(hipMemcpyAsync(d_o, m->d_obs_quads.get(), (size_t)ndata * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return st.finish();
}

int beatamd_ffi_variance_reductions_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, double *VR)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(Q && VR && C >= 0, BEATAMD_EINVAL, "ffi_variance_reductions: bad argument");
    BA_CHECK(!m->has_pol, BEATAMD_EINVAL,
             "the polarity composite has no Gaussian misfit: variance reductions are not defined for it");
    BA_TRY(model_check_layout(*m));
    const int64_t ndata = model_ndata(*m), nterm = model_nterm(*m);
    if (C == 0 || ndata == 0) return BEATAMD_OK;
    BA_TRY(model_obs_quads(ctx, *m));
    Staging st(ctx);
    const double *d_q;
    double *d_v;
    LogpOpts opt;
    BA_TRY(st.in(Q, (size_t)C * m->layout.nparams, &d_q));
    BA_TRY(st.out(VR, (size_t)C * ndata, &d_v));
    BA_TRY(ctx->scratch(SL_LPROP, (size_t)C * nterm, &opt.llks));
    BA_TRY(ffi_logp_device(ctx, *m, C, d_q, nullptr, opt));
    BA_TRY(launch_variance_reduction(ctx, C, ndata, opt.llks, nterm, m->d_obs_quads.get(), d_v));
    return st.finish();
}

int beatamd_ffi_geo_residuals_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, const double *Q, int32_t residuals,
                                    double *out)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(Q && out && C >= 0, BEATAMD_EINVAL, "ffi_geo_residuals: bad argument");
    BA_CHECK(m->has_geo, BEATAMD_EINVAL, "ffi_geo_residuals: the model has no geodetic composite");
    BA_TRY(model_check_layout(*m));
    if (C == 0) return BEATAMD_OK;
    const int64_t Nobs = m->geo.Nobs;
    Staging st(ctx);
    const double *d_q;
    double *d_o;
    BA_TRY(st.in(Q, (size_t)C * m->layout.nparams, &d_q));
    BA_TRY(st.out(out, (size_t)C * Nobs, &d_o));
    double *mu = d_o;   // (library mode keeps the synthetics apart from the residuals it makes of them)
    if (residuals && !m->geo_is_geometry) BA_TRY(ctx->scratch(SL_MU, (size_t)C * Nobs, &mu));
    BA_TRY(geodetic_residual(ctx, *m, C, d_q, mu, residuals ? d_o : nullptr));
    return st.finish();
}

int beatamd_standardize_batch(beatamd_ctx *ctx, int32_t kind, const double *S, int64_t T, int64_t N, int64_t C,
                              const double *R, const double *hp, double *out)
{
    ENTER(ctx);
    BA_CHECK(kind == BEATAMD_W_SCALAR || kind == BEATAMD_W_DENSE, BEATAMD_EINVAL, "unknown operator kind %d", kind);
    BA_CHECK(S && R && out && T > 0 && N > 0 && C >= 0, BEATAMD_EINVAL, "standardize: bad argument");
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_s, *d_r, *d_h;
    double *d_o;
    BA_TRY(st.in(S, (size_t)(kind == BEATAMD_W_SCALAR ? T : T * N * N), &d_s));
    BA_TRY(st.in(R, (size_t)C * T * N, &d_r));
    BA_TRY(st.in(hp, (size_t)C * T, &d_h));
    BA_TRY(st.out(out, (size_t)C * T * N, &d_o));
    if (kind == BEATAMD_W_SCALAR) {
        BA_TRY(launch_standardize(ctx, C, T, N, d_s, d_h, d_r, d_o));
        return st.finish();
    }
    BA_CHECK(d_o != d_r, BEATAMD_EINVAL, "standardize: a dense operator needs out apart from R");
    // out[c, t, :] = S_t . R[c, t, :]: per dataset the chains' rows times S_t^T, the datasets as the batch of one launch
    for (int64_t t0 = 0; t0 < T; t0 += 65535) {
        GemmCall g;
        g.A = d_r + t0 * N; g.lda = T * N; g.sA = N;
        g.B = d_s + t0 * N * N; g.ldb = N; g.sB = N * N; g.b_kn = 0;
        g.O = d_o + t0 * N; g.ldo = T * N; g.sO = N;
        g.M = C; g.N = N; g.K = N;
        g.nbatch = (int)std::min<int64_t>(65535, T - t0);
        g.timer = "standardize";
        BA_TRY(launch_gemm_f64(ctx, g));
    }
    if (d_h) BA_TRY(launch_standardize(ctx, C, T, N, nullptr, d_h, d_o, d_o));
    return st.finish();
}

static int pole_term_arg(const int64_t *off, const double *fixed, const double *earth, int64_t nparams, PoleTerm *t,
                         const char *who)
{
    for (int k = 0; k < 3; k++) {
        BA_CHECK(off[k] >= -1 && off[k] < nparams, BEATAMD_EINVAL, "%s: offset %lld of variable %d outside q", who,
                 (long long)off[k], k);
        t->off[k] = off[k];
        t->fix[k] = fixed[k];
        t->earth[k] = earth[k];
    }
    BA_CHECK(earth[0] > 0.0 && earth[1] > 0.0 && earth[2] >= 0.0 && earth[2] < 1.0, BEATAMD_EINVAL,
             "%s: earth (radius %g, equator radius %g, oblateness %g)", who, earth[0], earth[1], earth[2]);
    return BEATAMD_OK;
}

int beatamd_pole_coefficients_batch(beatamd_ctx *ctx, int64_t C, int64_t nparams, const double *Q, int32_t npole,
                                    const int64_t *var_off, const double *var_fixed, const double *earth, double *out)
{
    ENTER(ctx);
    BA_CHECK(C >= 0 && nparams > 0 && npole >= 1 && npole <= GEO_CORR_MAX && Q && var_off && var_fixed && earth && out,
             BEATAMD_EINVAL, "pole_coefficients_batch: bad argument");
    if (C == 0) return BEATAMD_OK;
    std::vector<int64_t> off;
    std::vector<double> fix, ea;
    BA_TRY(host_copy(ctx, var_off, (size_t)npole * 3, off));
    BA_TRY(host_copy(ctx, var_fixed, (size_t)npole * 3, fix));
    BA_TRY(host_copy(ctx, earth, (size_t)npole * 3, ea));
    std::vector<PoleTerm> terms((size_t)npole);
    for (int j = 0; j < npole; j++)
        BA_TRY(pole_term_arg(&off[(size_t)j * 3], &fix[(size_t)j * 3], &ea[(size_t)j * 3], nparams, &terms[(size_t)j],
                             "pole_coefficients_batch"));
    DevMem<PoleTerm> d_terms;
    BA_TRY(d_terms.alloc_copy(ctx, terms.data(), terms.size()));
    Staging st(ctx);
    const double *d_q;
    double *d_o;
    BA_TRY(st.in(Q, (size_t)C * nparams, &d_q));
    BA_TRY(st.out(out, (size_t)C * npole * 4, &d_o));
    BA_TRY(launch_pole_coef(ctx, d_terms.get(), npole, d_q, nparams, C, d_o));
    BA_TRY(st.finish());
    BA_HIP(hipStreamSynchronize(ctx->stream));   // (the term table goes with this call)
    return BEATAMD_OK;
}

int beatamd_pole_coupling_batch(beatamd_ctx *ctx, int64_t C, int64_t nparams, const double *Q, const int64_t *var_off,
                                const double *var_fixed, const double *earth, int64_t P, const double *Bp, int64_t uparr_off,
                                double *euler_slips, double *coupling)
{
    ENTER(ctx);
    BA_CHECK(C >= 0 && nparams > 0 && P >= 1 && Q && var_off && var_fixed && earth && Bp && euler_slips && coupling,
             BEATAMD_EINVAL, "pole_coupling_batch: bad argument");
    BA_CHECK(uparr_off >= 0 && uparr_off + P <= nparams, BEATAMD_EINVAL,
             "pole_coupling_batch: uparr [%lld, %lld) outside q of %lld", (long long)uparr_off, (long long)(uparr_off + P),
             (long long)nparams);
    if (C == 0) return BEATAMD_OK;
    std::vector<int64_t> off;
    std::vector<double> fix, ea;
    BA_TRY(host_copy(ctx, var_off, 3, off));
    BA_TRY(host_copy(ctx, var_fixed, 3, fix));
    BA_TRY(host_copy(ctx, earth, 3, ea));
    PoleTerm term;
    BA_TRY(pole_term_arg(off.data(), fix.data(), ea.data(), nparams, &term, "pole_coupling_batch"));
    Staging st(ctx);
    const double *d_q, *d_b;
    double *d_e, *d_c;
    BA_TRY(st.in(Q, (size_t)C * nparams, &d_q));
    BA_TRY(st.in(Bp, (size_t)P * 3, &d_b));
    BA_TRY(st.out(euler_slips, (size_t)C * P, &d_e));
    BA_TRY(st.out(coupling, (size_t)C * P, &d_c));
    BA_TRY(launch_pole_coupling(ctx, term, d_q, nparams, C, P, d_b, uparr_off, d_e, d_c));
    return st.finish();
}

int beatamd_ensemble_moments_update(beatamd_ctx *ctx, int64_t C, int64_t M, const double *X, double *state, int64_t n_seen)
{
    ENTER(ctx);
    BA_CHECK(X && state && C >= 0 && M > 0 && n_seen >= 0, BEATAMD_EINVAL, "ensemble_moments_update: bad argument");
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_x;
    double *d_s;
    BA_TRY(st.in(X, (size_t)C * M, &d_x));
    BA_TRY(st.out(state, (size_t)5 * M, &d_s, n_seen > 0));
    BA_TRY(launch_ensemble_moments(ctx, C, M, d_x, d_s, n_seen));
    return st.finish();
}

int beatamd_ensemble_moments_finish(beatamd_ctx *ctx, int64_t M, const double *state, int64_t n, double *mean, double *std,
                                    double *min, double *max)
{
    ENTER(ctx);
    BA_CHECK(state && mean && std && min && max && M > 0 && n > 0, BEATAMD_EINVAL, "ensemble_moments_finish: bad argument");
    Staging st(ctx);
    const double *d_s;
    double *d_me, *d_sd, *d_mn, *d_mx;
    BA_TRY(st.in(state, (size_t)5 * M, &d_s));
    BA_TRY(st.out(mean, (size_t)M, &d_me));
    BA_TRY(st.out(std, (size_t)M, &d_sd));
    BA_TRY(st.out(min, (size_t)M, &d_mn));
    BA_TRY(st.out(max, (size_t)M, &d_mx));
    BA_TRY(launch_moments_finish(ctx, M, d_s, n, d_me, d_sd, d_mn, d_mx));
    return st.finish();
}

int beatamd_trace_density_update(beatamd_ctx *ctx, int64_t E, int64_t T, int64_t N, const double *Y, const double *tmin,
                                 double deltat, const double *extent, int64_t ny, int64_t nx, double linewidth, double *grid)
{
    ENTER(ctx);
    BA_CHECK(Y && tmin && extent && grid && E >= 0 && T >= 0 && N > 0 && ny > 0 && nx > 0, BEATAMD_EINVAL,
             "trace_density_update: bad argument");
    Staging st(ctx);
    const double *d_y, *d_t, *d_e;
    double *d_g;
    BA_TRY(st.in(Y, (size_t)E * T * N, &d_y));
    BA_TRY(st.in(tmin, (size_t)T, &d_t));
    BA_TRY(st.in(extent, (size_t)4 * T, &d_e));
    BA_TRY(st.out(grid, (size_t)T * ny * nx, &d_g, true));
    BA_TRY(launch_trace_density(ctx, E, T, N, d_y, d_t, deltat, d_e, ny, nx, linewidth, d_g));
    BA_TRY(st.finish());
    return ctx->check_status();   // (device arrays too: a line outside the grid is the caller's TypeError now, not later)
}

int beatamd_trace_density_update_ranges(beatamd_ctx *ctx, int64_t E, int64_t T, int64_t N, const double *Y, const double *tmin,
                                        double deltat, const double *extent, const int64_t *ranges, int64_t ny, int64_t nx,
                                        double linewidth, double *grid)
{
    ENTER(ctx);
    BA_CHECK(Y && tmin && extent && grid && E >= 0 && T >= 0 && N > 0 && ny > 0 && nx > 0, BEATAMD_EINVAL,
             "trace_density_update_ranges: bad argument");
    Staging st(ctx);
    const double *d_y, *d_t, *d_e;
    const int64_t *d_r = nullptr;
    double *d_g;
    BA_TRY(st.in(Y, (size_t)E * T * N, &d_y));
    BA_TRY(st.in(tmin, (size_t)T, &d_t));
    BA_TRY(st.in(extent, (size_t)4 * T, &d_e));
    if (ranges) BA_TRY(st.in(ranges, (size_t)E * T * 2, &d_r));
    BA_TRY(st.out(grid, (size_t)T * ny * nx, &d_g, true));
    BA_TRY(launch_trace_density(ctx, E, T, N, d_y, d_t, deltat, d_e, ny, nx, linewidth, d_g, d_r));
    BA_TRY(st.finish());
    return ctx->check_status();
}

// ------------------------------------------------------------------ rupture fronts (rupture.hip)
// the subfault table on the host, checked: shapes, the blocks inside the start times and the coordinate arrays
static int rupture_subs(beatamd_ctx *ctx, const char *who, int32_t nsub, const int64_t *subs, int64_t ncells_total, int64_t nx_total,
                        int64_t ny_total, std::vector<int64_t> &sb, int64_t *max_nodes)
{
    BA_CHECK(subs && nsub >= 1 && nsub <= 4096 && ncells_total >= 0, BEATAMD_EINVAL, "%s: bad subfault table", who);
    BA_TRY(host_copy(ctx, subs, (size_t)nsub * CT_SUB_FIELDS, sb));
    *max_nodes = 0;
    for (int32_t k = 0; k < nsub; k++) {
        const int64_t *r = sb.data() + (size_t)CT_SUB_FIELDS * k;
        BA_CHECK(r[0] >= 1 && r[1] >= 1 && r[0] <= 32768 && r[1] <= 32768, BEATAMD_EINVAL, "%s: subfault %d of %lld x %lld patches",
                 who, (int)k, (long long)r[0], (long long)r[1]);
        BA_CHECK(r[2] >= 0 && r[2] + r[0] * r[1] <= ncells_total, BEATAMD_EINVAL,
                 "%s: subfault %d's patches [%lld, %lld) outside the %lld start times of a draw", who, (int)k, (long long)r[2],
                 (long long)(r[2] + r[0] * r[1]), (long long)ncells_total);
        BA_CHECK(nx_total < 0 || (r[3] >= 0 && r[3] + r[1] <= nx_total && r[4] >= 0 && r[4] + r[0] <= ny_total), BEATAMD_EINVAL,
                 "%s: subfault %d's coordinates outside x (%lld) or y (%lld)", who, (int)k, (long long)nx_total, (long long)ny_total);
        *max_nodes = std::max(*max_nodes, r[0] * r[1]);
    }
    return BEATAMD_OK;
}

int beatamd_rupture_minmax(beatamd_ctx *ctx, int64_t E, int64_t ncells_total, const double *sts, int32_t nsub, const int64_t *subs,
                           double *out)
{
    ENTER(ctx);
    BA_CHECK(sts && out && E >= 0, BEATAMD_EINVAL, "rupture_minmax: bad argument");
    std::vector<int64_t> sb;
    int64_t max_nodes = 0;
    BA_TRY(rupture_subs(ctx, "rupture_minmax", nsub, subs, ncells_total, -1, -1, sb, &max_nodes));
    if (E == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_s;
    const int64_t *d_sb;
    double *d_o;
    BA_TRY(st.in(sts, (size_t)E * ncells_total, &d_s));
    BA_TRY(st.in(subs, (size_t)nsub * CT_SUB_FIELDS, &d_sb));
    BA_TRY(st.out(out, (size_t)E * nsub * 2, &d_o));
    BA_TRY(launch_rupture_minmax(ctx, E, ncells_total, d_s, nsub, d_sb, d_o));
    return st.finish();
}

int beatamd_contour_count(beatamd_ctx *ctx, int64_t E, int64_t ncells_total, const double *sts, int32_t nsub, const int64_t *subs,
                          const double *levels, const int32_t *nlevels, int32_t *counts)
{
    ENTER(ctx);
    BA_CHECK(sts && levels && nlevels && counts && E >= 0, BEATAMD_EINVAL, "contour_count: bad argument");
    std::vector<int64_t> sb;
    std::vector<int32_t> nl;
    int64_t max_nodes = 0;
    BA_TRY(rupture_subs(ctx, "contour_count", nsub, subs, ncells_total, -1, -1, sb, &max_nodes));
    if (E == 0) return BEATAMD_OK;
    BA_TRY(host_copy(ctx, nlevels, (size_t)E * nsub, nl));
    for (size_t k = 0; k < nl.size(); k++)
        BA_CHECK(nl[k] >= 0 && nl[k] <= CT_LMAX, BEATAMD_EINVAL, "contour_count: %d levels for draw %lld (at most %d)", (int)nl[k],
                 (long long)(k / nsub), CT_LMAX);
    Staging st(ctx);
    const double *d_s, *d_l;
    const int64_t *d_sb;
    const int32_t *d_n;
    int32_t *d_c;
    BA_TRY(st.in(sts, (size_t)E * ncells_total, &d_s));
    BA_TRY(st.in(subs, (size_t)nsub * CT_SUB_FIELDS, &d_sb));
    BA_TRY(st.in(levels, (size_t)E * nsub * CT_LMAX, &d_l));
    BA_TRY(st.in(nlevels, (size_t)E * nsub, &d_n));
    BA_TRY(st.out(counts, (size_t)E * nsub * CT_LMAX * 2, &d_c));
    BA_TRY(launch_contours(ctx, E, ncells_total, d_s, nsub, d_sb, max_nodes, nullptr, nullptr, d_l, d_n, d_c, nullptr, nullptr, 0, 0,
                           nullptr, nullptr));
    return st.finish();
}

int beatamd_contour_fill(beatamd_ctx *ctx, int64_t E, int64_t ncells_total, const double *sts, int32_t nsub, const int64_t *subs,
                         int64_t nx_total, const double *x, int64_t ny_total, const double *y, const double *levels,
                         const int32_t *nlevels, const int64_t *line_base, const int64_t *vert_base, int64_t nlines, int64_t nverts,
                         double *vertices, int64_t *line_offsets)
{
    ENTER(ctx);
    BA_CHECK(sts && x && y && levels && nlevels && line_base && vert_base && vertices && line_offsets && E >= 0 && nlines >= 0 &&
             nverts >= 0 && nx_total >= 0 && ny_total >= 0, BEATAMD_EINVAL, "contour_fill: bad argument");
    std::vector<int64_t> sb, lb, vb;
    std::vector<int32_t> nl;
    int64_t max_nodes = 0;
    BA_TRY(rupture_subs(ctx, "contour_fill", nsub, subs, ncells_total, nx_total, ny_total, sb, &max_nodes));
    if (E == 0) return BEATAMD_OK;
    // the bases are the caller's scan of beatamd_contour_count's output: non-decreasing and inside the arrays they index.
    // The kernel writes what it counts again from the same start times, so a level's lines end where the next begin
    const size_t W = (size_t)E * nsub * CT_LMAX;
    BA_TRY(host_copy(ctx, line_base, W, lb));
    BA_TRY(host_copy(ctx, vert_base, W, vb));
    BA_TRY(host_copy(ctx, nlevels, (size_t)E * nsub, nl));
    for (size_t k = 0; k < W; k++) {
        BA_CHECK(lb[k] >= 0 && lb[k] <= nlines && vb[k] >= 0 && vb[k] <= nverts && (k == 0 || (lb[k] >= lb[k - 1] && vb[k] >= vb[k - 1])),
                 BEATAMD_EINVAL, "contour_fill: line_base / vert_base are not the scans of contour_count's counts");
        const size_t cap = 2 * (size_t)max_nodes;     // (a level has at most two segments a cell, each at most two vertices)
        BA_CHECK((k + 1 < W ? (size_t)(vb[k + 1] - vb[k]) : (size_t)(nverts - vb[k])) <= 2 * cap, BEATAMD_EINVAL,
                 "contour_fill: a level with more vertices than its subfault can give");
    }
    for (size_t k = 0; k < nl.size(); k++)
        BA_CHECK(nl[k] >= 0 && nl[k] <= CT_LMAX, BEATAMD_EINVAL, "contour_fill: %d levels for draw %lld (at most %d)", (int)nl[k],
                 (long long)(k / nsub), CT_LMAX);
    Staging st(ctx);
    const double *d_s, *d_l, *d_x, *d_y;
    const int64_t *d_sb, *d_lb, *d_vb;
    const int32_t *d_n;
    double *d_v;
    int64_t *d_lo;
    BA_TRY(st.in(sts, (size_t)E * ncells_total, &d_s));
    BA_TRY(st.in(subs, (size_t)nsub * CT_SUB_FIELDS, &d_sb));
    BA_TRY(st.in(x, (size_t)nx_total, &d_x));
    BA_TRY(st.in(y, (size_t)ny_total, &d_y));
    BA_TRY(st.in(levels, W, &d_l));
    BA_TRY(st.in(nlevels, (size_t)E * nsub, &d_n));
    BA_TRY(st.in(line_base, W, &d_lb));
    BA_TRY(st.in(vert_base, W, &d_vb));
    BA_TRY(st.out(vertices, (size_t)nverts * 2, &d_v));
    BA_TRY(st.out(line_offsets, (size_t)nlines + 1, &d_lo, true));
    BA_TRY(launch_contours(ctx, E, ncells_total, d_s, nsub, d_sb, max_nodes, d_x, d_y, d_l, d_n, nullptr, d_lb, d_vb, nlines, nverts, d_v,
                           d_lo));
    return st.finish();
}

int beatamd_polyline_density(beatamd_ctx *ctx, int64_t nverts, const double *vertices, int64_t nlines, const int64_t *line_offsets,
                             int64_t nsel, const int64_t *sel, const double *extent, int64_t ny, int64_t nx, double linewidth,
                             double *grid, int32_t *coverage)
{
    ENTER(ctx);
    BA_CHECK(line_offsets && extent && grid && nverts >= 0 && nlines >= 0 && nsel >= 0 && ny > 0 && nx > 0 && (vertices || !nverts),
             BEATAMD_EINVAL, "polyline_density: bad argument");
    // the offsets and the selection index device arrays: checked here, on the host
    std::vector<int64_t> lo, se;
    std::vector<double> ext;
    BA_TRY(host_copy(ctx, line_offsets, (size_t)nlines + 1, lo));
    BA_TRY(host_copy(ctx, extent, 4, ext));
    BA_CHECK(lo[0] >= 0 && lo[nlines] <= nverts, BEATAMD_EINDEX, "polyline_density: line_offsets [%lld, %lld] outside %lld vertices",
             (long long)lo[0], (long long)lo[nlines], (long long)nverts);
    for (int64_t k = 0; k < nlines; k++)
        BA_CHECK(lo[k] <= lo[k + 1], BEATAMD_EINDEX, "polyline_density: line_offsets decrease at line %lld", (long long)k);
    if (sel) {
        BA_TRY(host_copy(ctx, sel, (size_t)nsel, se));
        for (int64_t k = 0; k < nsel; k++)
            BA_CHECK(se[k] >= 0 && se[k] < nlines, BEATAMD_EINDEX, "polyline_density: polyline %lld of %lld", (long long)se[k],
                     (long long)nlines);
    } else {
        BA_CHECK(nsel == nlines, BEATAMD_EINVAL, "polyline_density: no selection, but %lld of %lld polylines", (long long)nsel,
                 (long long)nlines);
    }
    Staging st(ctx);
    const double *d_v;
    const int64_t *d_lo, *d_se = nullptr;
    double *d_g;
    int32_t *d_c = nullptr;
    BA_TRY(st.in(vertices, (size_t)nverts * 2, &d_v));
    BA_TRY(st.in(line_offsets, (size_t)nlines + 1, &d_lo));
    if (sel) BA_TRY(st.in(sel, (size_t)nsel, &d_se));
    BA_TRY(st.out(grid, (size_t)ny * nx, &d_g, true));
    if (coverage) BA_TRY(st.out(coverage, (size_t)ny * nx, &d_c, true));
    BA_TRY(launch_polyline_density(ctx, nsel, d_se, d_lo, d_v, ext.data(), ny, nx, linewidth, d_g, d_c));
    BA_TRY(st.finish());
    return ctx->check_status();   // (device arrays too: a line outside the grid is the caller's TypeError now, not later)
}

// ------------------------------------------------------------------ the hyper-parameter model (hyper.hip)
int beatamd_hyper_model_create(beatamd_ctx *ctx, int64_t nterm, int64_t nh, const int64_t *M, const double *slog,
                               const int32_t *kind, const int32_t *hp_index, int32_t ngroups, const int32_t *group_end,
                               int32_t *id)
{
    ENTER(ctx);
    BA_CHECK(M && slog && kind && hp_index && group_end && id && nterm > 0 && nh > 0 && ngroups >= 1 && ngroups <= 8,
             BEATAMD_EINVAL, "hyper_model_create: bad argument");
    BA_CHECK(nterm <= 2048, BEATAMD_EINVAL, "hyper_model_create: %lld terms (at most 2048)", (long long)nterm);
    std::vector<double> Md((size_t)nterm);
    for (int64_t k = 0; k < nterm; k++) {
        BA_CHECK(kind[k] == 0 || kind[k] == 1, BEATAMD_EINVAL, "hyper_model_create: term %lld: kind must be 0 (dataset) or 1 "
                 "(Laplacian)", (long long)k);
        BA_CHECK(hp_index[k] >= 0 && hp_index[k] < nh, BEATAMD_EINVAL, "hyper_model_create: term %lld: hyper-parameter %d of %lld",
                 (long long)k, hp_index[k], (long long)nh);
        Md[k] = (double)M[k];
    }
    auto h = std::make_unique<HyperModel>();
    h->nterm = nterm; h->nh = nh; h->ngroups = ngroups;
    for (int g = 0; g < ngroups; g++) {
        BA_CHECK(group_end[g] > 0 && group_end[g] <= nterm && (g == 0 || group_end[g] >= group_end[g - 1]), BEATAMD_EINVAL,
                 "hyper_model_create: composite boundaries must ascend inside the term vector");
        h->group_end[g] = group_end[g];
    }
    BA_CHECK(group_end[ngroups - 1] == nterm, BEATAMD_EINVAL, "hyper_model_create: the last composite ends at nterm");
    BA_TRY(h->M.alloc_copy(ctx, Md.data(), (size_t)nterm));
    BA_TRY(h->slog.alloc_copy(ctx, slog, (size_t)nterm));
    BA_TRY(h->kind.alloc_copy(ctx, kind, (size_t)nterm));
    BA_TRY(h->hp_index.alloc_copy(ctx, hp_index, (size_t)nterm));
    *id = add_obj(ctx->hypers, std::move(h));
    return BEATAMD_OK;
}

int beatamd_hyper_model_destroy(beatamd_ctx *ctx, int32_t id)
{
    ENTER(ctx);
    return destroy_obj(ctx, ctx->hypers, id, "hyper model");
}

int beatamd_hyper_logp_batch(beatamd_ctx *ctx, int32_t id, int64_t C, const double *H, const double *llks, double *LL)
{
    ENTER(ctx);
    HyperModel *h;
    BA_TRY(find_hyper(ctx, id, &h));
    BA_CHECK(H && llks && LL && C >= 0, BEATAMD_EINVAL, "hyper_logp: bad argument");
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_h, *d_l;
    double *d_o;
    BA_TRY(st.in(H, (size_t)C * h->nh, &d_h));
    BA_TRY(st.in(llks, (size_t)C * h->nterm, &d_l));
    BA_TRY(st.out(LL, (size_t)C * (h->nterm + 1), &d_o));
    BA_TRY(launch_hyper_logp(ctx, *h, C, d_h, d_l, d_o));
    return st.finish();
}

int beatamd_hyper_chain_batch(beatamd_ctx *ctx, int32_t id, int64_t C, int64_t n_steps, double *H, double *LL,
                              double *scaling, int32_t *accepted_since_tune, const double *llks, const double *lower,
                              const double *upper, int32_t kind, const double *scales, uint64_t seed, uint32_t step0,
                              int64_t first_chain, int32_t tune_interval, int32_t steps_until_tune, int32_t buffer_thinning,
                              double *trace, int64_t *n_accepted)
{
    ENTER(ctx);
    HyperModel *h;
    BA_TRY(find_hyper(ctx, id, &h));
    BA_CHECK(H && LL && scaling && accepted_since_tune && llks && lower && upper && scales && C >= 0 && n_steps >= 0 &&
             first_chain >= 0 && tune_interval >= 0 && buffer_thinning >= 1, BEATAMD_EINVAL, "hyper_chain: bad argument");
    BA_CHECK(tune_interval == 0 || (steps_until_tune >= 0 && steps_until_tune <= tune_interval), BEATAMD_EINVAL,
             "hyper_chain: steps_until_tune must lie in [0, tune_interval]");
    BA_CHECK(kind >= BEATAMD_PROPOSAL_NORMAL && kind <= BEATAMD_PROPOSAL_LAPLACE, BEATAMD_EINVAL,
             "hyper_chain: kind must be Normal (0), Cauchy (1) or Laplace (2)");
    BA_CHECK(hyper_chain_applicable(h->nh, h->nterm), BEATAMD_EINVAL,
             "hyper_chain: %lld hyper-parameters / %lld terms exceed what a chain's wavefront holds (%d each): take the "
             "step-by-step path", (long long)h->nh, (long long)h->nterm, HYPER_CHAIN_MAX);
    BA_CHECK(is_device_ptr(H) && is_device_ptr(LL) && is_device_ptr(scaling) && is_device_ptr(accepted_since_tune) &&
             is_device_ptr(llks) && is_device_ptr(lower) && is_device_ptr(upper) && is_device_ptr(scales) &&
             (!trace || is_device_ptr(trace)) && (!n_accepted || is_device_ptr(n_accepted)), BEATAMD_EINVAL,
             "hyper_chain: device pointers only");
    HyperChainCall k;
    k.C = C; k.n_steps = n_steps; k.H = H; k.LL = LL; k.scaling = scaling; k.acc_since = accepted_since_tune;
    k.llks = llks; k.lower = lower; k.upper = upper; k.scales = scales; k.kind = kind; k.seed = seed;
    k.first_chain = (uint64_t)first_chain; k.step0 = step0; k.tune_interval = tune_interval;
    k.steps_until_tune = steps_until_tune; k.buffer_thinning = buffer_thinning; k.trace = trace; k.n_acc = n_accepted;
    return launch_hyper_chain(ctx, *h, k);
}

// the three step entry points: the model of the id, then astep_impl (model.cpp)
static int astep_entry(beatamd_ctx *ctx, int32_t model_id, int64_t C, double *Q0, double *L0, const double *delta,
                       const double *scaling, const double *lower, const double *upper, const double *log_u, double beta,
                       const double *betas, int32_t *accepted, const StepDraw *draw = nullptr, int32_t *acc_sum = nullptr,
                       int64_t *n_acc = nullptr)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    return astep_impl(ctx, *m, C, Q0, L0, delta, scaling, lower, upper, log_u, beta, betas, accepted, draw, acc_sum, n_acc);
}

int beatamd_ffi_astep_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, double *Q0, double *L0,
                            const double *delta, const double *scaling, const double *lower,
                            const double *upper, const double *log_u, double beta,
                            int32_t *accepted)
{
    return astep_entry(ctx, model_id, C, Q0, L0, delta, scaling, lower, upper, log_u, beta, nullptr, accepted);
}

int beatamd_ffi_astep_batch_betas(beatamd_ctx *ctx, int32_t model_id, int64_t C, double *Q0,
                                  double *L0, const double *delta, const double *scaling,
                                  const double *lower, const double *upper, const double *log_u,
                                  const double *betas, int32_t *accepted)
{
    BA_CHECK(ctx != nullptr && betas != nullptr, BEATAMD_EINVAL, "ffi_astep_betas: NULL argument");
    return astep_entry(ctx, model_id, C, Q0, L0, delta, scaling, lower, upper, log_u, 1.0, betas, accepted);
}

int beatamd_ffi_mstep_batch(beatamd_ctx *ctx, int32_t model_id, int64_t C, double *Q0, double *L0,
                            const double *factor, int64_t K, int32_t kind, int32_t df, uint64_t seed,
                            uint32_t step, int64_t first_chain, const double *scaling, const double *lower,
                            const double *upper, double beta, const double *betas, int32_t *accepted,
                            int32_t *accepted_sum, int64_t *n_accepted)
{
    BA_CHECK(ctx != nullptr, BEATAMD_EINVAL, "ctx is NULL");
    BA_CHECK(factor && first_chain >= 0 && df >= 0 && df <= 64, BEATAMD_EINVAL, "ffi_mstep: bad argument");
    BA_CHECK(kind >= -1 && kind <= BEATAMD_PROPOSAL_POISSON && (kind >= 0 || K > 0), BEATAMD_EINVAL,
             "ffi_mstep: kind must be -1 (multivariate, K > 0 factor rows), Normal (0), Cauchy (1), Laplace (2) or "
             "Poisson (3)");
    StepDraw d;
    d.factor = factor; d.K = K; d.kind = kind; d.df = kind < 0 ? df : 0;
    d.seed = seed; d.step = step; d.first_chain = (uint64_t)first_chain;
    return astep_entry(ctx, model_id, C, Q0, L0, nullptr, scaling, lower, upper, nullptr, betas ? 1.0 : beta, betas, accepted,
                       &d, accepted_sum, n_accepted);
}

int beatamd_ffi_mstep_batch_grouped(beatamd_ctx *ctx, int32_t model_id, int64_t C, int64_t G, double *Q0, double *L0,
                                    const double *factor, int64_t K, int32_t df, uint64_t seed, uint32_t step,
                                    int64_t first_chain, const double *scaling, const double *lower, const double *upper,
                                    double beta, const double *betas, int32_t *accepted, int32_t *accepted_sum,
                                    int64_t *n_accepted)
{
    BA_CHECK(ctx != nullptr, BEATAMD_EINVAL, "ctx is NULL");
    BA_CHECK(factor && first_chain >= 0 && df >= 0 && df <= 64 && K > 0, BEATAMD_EINVAL, "ffi_mstep_grouped: bad argument");
    BA_CHECK(G >= 1 && G <= 65535 && C >= 0 && C % G == 0, BEATAMD_EINVAL,
             "ffi_mstep_grouped: %lld chains do not fall into %lld equal groups", (long long)C, (long long)G);
    StepDraw d;
    d.factor = factor; d.K = K; d.kind = -1; d.df = df; d.groups = G;
    d.seed = seed; d.step = step; d.first_chain = (uint64_t)first_chain;
    return astep_entry(ctx, model_id, C, Q0, L0, nullptr, scaling, lower, upper, nullptr, betas ? 1.0 : beta, betas, accepted,
                       &d, accepted_sum, n_accepted);
}

// ------------------------------------------------------------------ noise covariance
int beatamd_autocovariance_batch(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *data,
                                 const double *mean, double *out)
{
    ENTER(ctx);
    BA_CHECK(data && out && nd >= 0 && n >= 0, BEATAMD_EINVAL, "autocovariance: bad argument");
    if (nd == 0 || n == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_d, *d_m;
    double *d_o;
    BA_TRY(st.in(data, (size_t)nd * n, &d_d));
    BA_TRY(st.in(mean, (size_t)nd, &d_m));
    BA_TRY(st.out(out, (size_t)nd * n, &d_o));
    BA_TRY(launch_autocovariance(ctx, nd, n, d_d, d_m, d_o));
    return st.finish();
}

int beatamd_scaled_toeplitz_batch(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *coeffs,
                                  const double *stds, double *out)
{
    ENTER(ctx);
    BA_CHECK(coeffs && stds && out && nd >= 0 && n >= 0, BEATAMD_EINVAL, "scaled_toeplitz: bad argument");
    if (nd == 0 || n == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_c, *d_s;
    double *d_o;
    BA_TRY(st.in(coeffs, (size_t)nd * n, &d_c));
    BA_TRY(st.in(stds, (size_t)nd * n, &d_s));
    BA_TRY(st.out(out, (size_t)nd * n * n, &d_o));
    BA_TRY(launch_scaled_toeplitz(ctx, nd, n, d_c, d_s, d_o));
    return st.finish();
}

int beatamd_ball_rms_batch(beatamd_ctx *ctx, int64_t nd, const int64_t *sizes, const double *coords, const double *data,
                           double max_dist_perc, double *radius, int32_t *counts, double *stds)
{
    ENTER(ctx);
    BA_CHECK(sizes && coords && data && radius && counts && stds, BEATAMD_EINVAL, "ball_rms_batch: NULL array");
    BA_CHECK(nd > 0 && nd <= 65535, BEATAMD_EINVAL, "ball_rms_batch: 1..65535 datasets, got %lld", (long long)nd);
    BA_CHECK(std::isfinite(max_dist_perc), BEATAMD_EINVAL, "ball_rms_batch: max_dist_perc is not finite");
    std::vector<int64_t> n;
    BA_TRY(host_copy(ctx, sizes, (size_t)nd, n));
    std::vector<BallSet> sets((size_t)nd);
    int64_t total = 0, nmax = 0;
    for (int64_t i = 0; i < nd; i++) {
        BA_CHECK(n[i] > 0, BEATAMD_EINVAL, "ball_rms_batch: dataset %lld has %lld points", (long long)i, (long long)n[i]);
        sets[(size_t)i] = BallSet{total, n[i]};
        total += n[i];
        nmax = std::max(nmax, n[i]);
    }
    Staging st(ctx);
    const double *d_c, *d_d;
    double *d_r, *d_s, *d_pmax;
    int32_t *d_n;
    BallSet *d_sets;
    BA_TRY(st.in(coords, (size_t)total * 2, &d_c));
    BA_TRY(st.in(data, (size_t)total, &d_d));
    BA_TRY(st.out(radius, (size_t)nd, &d_r));
    BA_TRY(st.out(counts, (size_t)total, &d_n));
    BA_TRY(st.out(stds, (size_t)total, &d_s));
    BA_TRY(ctx->scratch(SL_PARTIAL, (size_t)total, &d_pmax));
    BA_TRY(ctx->scratch(SL_MISC, (size_t)nd, &d_sets));
    BA_HIP(hipMemcpyAsync(d_sets, sets.data(), sets.size() * sizeof(BallSet), hipMemcpyHostToDevice, ctx->stream));
    BA_TRY(launch_ball_rms(ctx, nd, nmax, d_sets, d_c, d_d, max_dist_perc, d_pmax, d_r, d_n, d_s));
    // the table is this call's: the stream is drained before it goes
    BA_HIP(hipStreamSynchronize(ctx->stream));
    return st.finish();
}

// ------------------------------------------------------------------ introspection
int beatamd_ctx_last_kernel(beatamd_ctx *ctx, char *buf, int64_t buflen)
{
    BA_CHECK(ctx && buf && buflen > 0, BEATAMD_EINVAL, "last_kernel: bad argument");
    snprintf(buf, (size_t)buflen, "%s", ctx->last_gf_kernel);
    return BEATAMD_OK;
}

int beatamd_ctx_gf_group_stats(beatamd_ctx *ctx, int64_t *chains_per_group, double *mean_rows,
                               int64_t *max_rows, int64_t *row_bytes)
{
    ENTER(ctx);
    BA_CHECK(chains_per_group && mean_rows && max_rows && row_bytes, BEATAMD_EINVAL,
             "gf_group_stats: NULL argument");
    *chains_per_group = ctx->gs_cg;
    *mean_rows = 0.0;
    *max_rows = 0;
    *row_bytes = 0;
    if (ctx->gs_ngtp == 0) return BEATAMD_OK;  // the last launch was the streaming kernel
    int64_t tot = 0;
    BA_TRY(gs_counters(ctx, 0, &tot, max_rows));
    *mean_rows = (double)tot / (double)ctx->gs_ngtp;
    // every distinct row is staged once per (group, target) and slip variable
    *row_bytes = (int64_t)((double)tot * ctx->gs_trep) * ctx->gs_N * 8 * ctx->gs_nvar;
    return BEATAMD_OK;
}

int beatamd_ctx_gf_plan(beatamd_ctx *ctx, char *buf, int64_t buflen, double *mean_passes, int64_t *max_passes)
{
    ENTER(ctx);
    BA_CHECK(buf && buflen > 0, BEATAMD_EINVAL, "gf_plan: bad argument");
    snprintf(buf, (size_t)buflen, "%s", ctx->gf_plan);
    if (mean_passes) *mean_passes = ctx->gs_ngtp ? 1.0 : 0.0;
    if (max_passes) *max_passes = ctx->gs_ngtp ? 1 : 0;
    if (!ctx->gs_has_passes || ctx->gs_ngtp == 0 || (!mean_passes && !max_passes)) return BEATAMD_OK;
    int64_t tot = 0, mx = 0;
    BA_TRY(gs_counters(ctx, 1, &tot, &mx));
    if (mean_passes) *mean_passes = (double)tot / (double)ctx->gs_ngtp;
    if (max_passes) *max_passes = mx;
    return BEATAMD_OK;
}

int beatamd_ctx_gf_tune_log(beatamd_ctx *ctx, char *buf, int64_t buflen)
{
    ENTER(ctx);
    BA_CHECK(buf && buflen > 0, BEATAMD_EINVAL, "gf_tune_log: bad argument");
    snprintf(buf, (size_t)buflen, "%s", ctx->gf_tune_log);
    return BEATAMD_OK;
}

int32_t beatamd_gf_patch_ranges(int64_t ntargets, int64_t npatches, int64_t nsamples, int32_t num_cu)
{
    if (ntargets <= 0 || npatches <= 0 || nsamples <= 0) return 1;
    return (int32_t)gf_patch_ranges(ntargets, npatches, nsamples, num_cu > 0 ? num_cu : 256);
}

int32_t beatamd_fast_sweep_lds(int32_t ncells, int32_t *waves)
{
    if (ncells <= 0 || ncells > SWEEP_MAX_CELLS) return -1;
    const SweepLdsPlan pl = sweep_lds_plan(ncells);
    if (waves) *waves = pl.waves;
    return (int32_t)pl.bytes;
}

int beatamd_ctx_gf_chain_groups(beatamd_ctx *ctx, int64_t C, const double *key0, const double *key1,
                                int64_t chains_per_group, uint32_t *members)
{
    ENTER(ctx);
    BA_CHECK(C > 0 && key0 && key1 && members && chains_per_group > 0, BEATAMD_EINVAL, "gf_chain_groups: bad argument");
    const int64_t ngroups = (C + chains_per_group - 1) / chains_per_group;
    const ChainVec key[2] = {ChainVec{key0, 1, 0}, ChainVec{key1, 1, 0}};
    const uint32_t *m = nullptr;
    BA_TRY(launch_chain_members(ctx, C, key, chains_per_group, ngroups, &m));
    BA_CHECK(m != nullptr, BEATAMD_EINVAL, "gf_chain_groups: groups of more than 8192 chains are not cut");
    BA_HIP(hipStreamSynchronize(ctx->stream));
    BA_HIP(hipMemcpy(members, m, (size_t)(ngroups * chains_per_group) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return BEATAMD_OK;
}

// ------------------------------------------------------------------ SMC stage transition
int beatamd_smc_calc_beta(beatamd_ctx *ctx, int64_t C, const double *likelihoods, int64_t stride,
                          double beta, double coef_variation, double *beta_new, double *weights)
{
    ENTER(ctx);
    BA_CHECK(likelihoods && beta_new && weights && C > 0 && stride > 0, BEATAMD_EINVAL,
             "smc_calc_beta: bad argument");
    // smc.py:152: the bisection runs while 2 - beta > 1e-6; past that the reference has no midpoint to return (it fails
    // on an unbound name) and the kernel would divide the weights by a total it never summed
    BA_CHECK(2.0 - beta > 1e-6, BEATAMD_EINVAL, "smc_calc_beta: beta = %g leaves no tempering step below 2", beta);
    Staging st(ctx);
    const double *d_l;
    double *d_w, *d_out;
    BA_TRY(st.in(likelihoods, (size_t)((C - 1) * stride + 1), &d_l));
    BA_TRY(st.out(weights, (size_t)C, &d_w));
    BA_TRY(ctx->scratch(SL_STAGE2, 8, &d_out));
    BA_TRY(launch_smc_calc_beta(ctx, C, d_l, stride, beta, coef_variation, 0, 0.0, d_out, d_w));
    double out[2];
    BA_HIP(hipMemcpyAsync(out, d_out, sizeof(out), hipMemcpyDeviceToHost, ctx->stream));
    BA_TRY(st.finish());
    BA_HIP(hipStreamSynchronize(ctx->stream));
    *beta_new = out[0];
    return BEATAMD_OK;
}

int beatamd_smc_stage_weights(beatamd_ctx *ctx, int64_t C, const double *likelihoods, int64_t stride,
                              double dbeta, double *weights)
{
    ENTER(ctx);
    BA_CHECK(likelihoods && weights && C > 0 && stride > 0, BEATAMD_EINVAL, "smc_stage_weights: bad argument");
    Staging st(ctx);
    const double *d_l;
    double *d_w, *d_out;
    BA_TRY(st.in(likelihoods, (size_t)((C - 1) * stride + 1), &d_l));
    BA_TRY(st.out(weights, (size_t)C, &d_w));
    BA_TRY(ctx->scratch(SL_STAGE2, 8, &d_out));
    BA_TRY(launch_smc_calc_beta(ctx, C, d_l, stride, 0.0, 0.0, 1, dbeta, d_out, d_w));
    return st.finish();
}

int beatamd_smc_resample(beatamd_ctx *ctx, int64_t C, const double *weights, double aux,
                         int32_t *indexes)
{
    ENTER(ctx);
    BA_CHECK(weights && indexes && C > 0, BEATAMD_EINVAL, "smc_resample: bad argument");
    BA_CHECK(C < (int64_t)0x7fffffff, BEATAMD_EINVAL, "smc_resample: too many chains");
    Staging st(ctx);
    const double *d_w;
    int32_t *d_i;
    double *cum;
    BA_TRY(st.in(weights, (size_t)C, &d_w));
    BA_TRY(st.out(indexes, (size_t)C, &d_i));
    BA_TRY(ctx->scratch(SL_CUM, (size_t)C, &cum));
    BA_TRY(launch_smc_resample(ctx, C, d_w, aux, cum, d_i));
    return st.finish();
}

int beatamd_smc_population_factor(beatamd_ctx *ctx, int64_t C, int64_t nparams,
                                  const double *population, const double *weights, double *factor)
{
    ENTER(ctx);
    BA_CHECK(population && weights && factor && C > 0 && nparams > 0, BEATAMD_EINVAL,
             "smc_population_factor: bad argument");
    Staging st(ctx);
    const double *d_x, *d_w;
    double *d_f;
    BA_TRY(st.in(population, (size_t)C * nparams, &d_x));
    BA_TRY(st.in(weights, (size_t)C, &d_w));
    BA_TRY(st.out(factor, (size_t)C * nparams, &d_f));
    BA_TRY(launch_pop_factor(ctx, C, nparams, d_x, nparams, d_w, d_f));
    return st.finish();
}

int beatamd_proposal_draw(beatamd_ctx *ctx, int64_t C, int64_t K, int64_t nparams,
                          const double *factor, uint64_t seed, uint32_t step, int64_t first_chain,
                          int32_t df, double *delta, double *log_u)
{
    ENTER(ctx);
    BA_CHECK(factor && delta && C >= 0 && K > 0 && nparams > 0 && df >= 0 && first_chain >= 0,
             BEATAMD_EINVAL, "proposal_draw: bad argument");
    BA_CHECK(df <= 64, BEATAMD_EINVAL, "proposal_draw: at most 64 degrees of freedom");
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_f;
    double *d_d, *d_u = nullptr;
    BA_TRY(st.in(factor, (size_t)K * nparams, &d_f));
    BA_TRY(st.out(delta, (size_t)C * nparams, &d_d));
    if (log_u) {
        BA_TRY(st.out(log_u, (size_t)C, &d_u));
    }
    BA_TRY(draw_multivariate(ctx, C, K, nparams, d_f, df, seed, step, (uint64_t)first_chain, d_d, d_u));
    BA_TRY(launch_step_advance(ctx));
    return st.finish();
}

int beatamd_proposal_draw_grouped(beatamd_ctx *ctx, int64_t C, int64_t G, int64_t K, int64_t nparams, const double *factor,
                                  uint64_t seed, uint32_t step, int64_t first_chain, int32_t df, double *delta, double *log_u)
{
    ENTER(ctx);
    BA_CHECK(factor && delta && C >= 0 && K > 0 && nparams > 0 && df >= 0 && df <= 64 && first_chain >= 0, BEATAMD_EINVAL,
             "proposal_draw_grouped: bad argument");
    BA_CHECK(G >= 1 && G <= 65535 && C % G == 0, BEATAMD_EINVAL,
             "proposal_draw_grouped: %lld chains do not fall into %lld equal groups", (long long)C, (long long)G);
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_f;
    double *d_d, *d_u = nullptr;
    BA_TRY(st.in(factor, (size_t)G * K * nparams, &d_f));
    BA_TRY(st.out(delta, (size_t)C * nparams, &d_d));
    if (log_u) {
        BA_TRY(st.out(log_u, (size_t)C, &d_u));
    }
    BA_TRY(draw_multivariate(ctx, C, K, nparams, d_f, df, seed, step, (uint64_t)first_chain, d_d, d_u, G));
    BA_TRY(launch_step_advance(ctx));
    return st.finish();
}

// ------------------------------------------------------------------ PT proposal adaptation (ptadapt.hip)
static int group_moments_shape(beatamd_ctx *ctx, const char *who, int64_t G, int64_t n)
{
    BA_CHECK(G >= 1 && G <= GM_MAX_G && n >= 1 && n <= GM_MAX_N, BEATAMD_EINVAL,
             "%s: 1..%d groups of 1..%d parameters, got %lld of %lld", who, GM_MAX_G, GM_MAX_N, (long long)G, (long long)n);
    return BEATAMD_OK;
}

int beatamd_group_moments_reset(beatamd_ctx *ctx, int64_t G, int64_t nparams, double *state, int64_t R, const double *Q,
                                double *ref)
{
    ENTER(ctx);
    BA_CHECK(state && (!ref || (Q && R >= 1 && R <= GM_MAX_R)), BEATAMD_EINVAL, "group_moments_reset: bad argument");
    BA_TRY(group_moments_shape(ctx, "group_moments_reset", G, nparams));
    Staging st(ctx);
    const double *d_q = nullptr;
    double *d_s, *d_r = nullptr;
    BA_TRY(st.out(state, (size_t)(G * group_moments_stride(nparams)), &d_s));
    if (ref) {
        BA_TRY(st.in(Q, (size_t)(G * R * nparams), &d_q));
        BA_TRY(st.out(ref, (size_t)(G * nparams), &d_r));
    }
    BA_TRY(launch_group_moments_reset(ctx, G, nparams, d_s, R, d_q, d_r));
    return st.finish();
}

int beatamd_group_moments_update(beatamd_ctx *ctx, int64_t G, int64_t R, int64_t nparams, const double *Q, const double *like,
                                 int64_t like_stride, const double *ref, double *state)
{
    ENTER(ctx);
    BA_CHECK(Q && like && ref && state && like_stride > 0, BEATAMD_EINVAL, "group_moments_update: bad argument");
    BA_TRY(group_moments_shape(ctx, "group_moments_update", G, nparams));
    BA_CHECK(R >= 1 && R <= GM_MAX_R, BEATAMD_EINVAL, "group_moments_update: 1..%d rows per group, got %lld", GM_MAX_R,
             (long long)R);
    Staging st(ctx);
    const double *d_q, *d_l, *d_r;
    double *d_s;
    BA_TRY(st.in(Q, (size_t)(G * R * nparams), &d_q));
    BA_TRY(st.in(like, (size_t)((G * R - 1) * like_stride + 1), &d_l));
    BA_TRY(st.in(ref, (size_t)(G * nparams), &d_r));
    BA_TRY(st.out(state, (size_t)(G * group_moments_stride(nparams)), &d_s, true));
    BA_TRY(launch_group_moments_update(ctx, G, R, nparams, d_q, d_l, like_stride, d_r, d_s));
    return st.finish();
}

int beatamd_group_moments_factor(beatamd_ctx *ctx, int64_t G, int64_t nparams, const double *state, double *factor,
                                 double *cov, int32_t *flags)
{
    ENTER(ctx);
    BA_CHECK(state && factor && flags, BEATAMD_EINVAL, "group_moments_factor: NULL argument");
    BA_TRY(group_moments_shape(ctx, "group_moments_factor", G, nparams));
    Staging st(ctx);
    const double *d_s;
    double *d_f, *d_c = nullptr;
    int32_t *d_fl;
    BA_TRY(st.in(state, (size_t)(G * group_moments_stride(nparams)), &d_s));
    BA_TRY(st.out(factor, (size_t)(G * nparams * nparams), &d_f, true));   // (a flagged group's factor stays as it is)
    if (cov) BA_TRY(st.out(cov, (size_t)(G * nparams * nparams), &d_c));
    BA_TRY(st.out(flags, (size_t)G, &d_fl));
    BA_TRY(launch_group_moments_factor(ctx, G, nparams, d_s, d_f, d_c, d_fl));
    return st.finish();
}

int beatamd_proposal_draw_univariate(beatamd_ctx *ctx, int64_t C, int64_t nparams, int32_t kind,
                                     const double *scale, uint64_t seed, uint32_t step, int64_t first_chain,
                                     double *delta, double *log_u)
{
    ENTER(ctx);
    BA_CHECK(scale && delta && C >= 0 && nparams > 0 && first_chain >= 0, BEATAMD_EINVAL,
             "proposal_draw_univariate: bad argument");
    BA_CHECK(kind >= BEATAMD_PROPOSAL_NORMAL && kind <= BEATAMD_PROPOSAL_POISSON, BEATAMD_EINVAL,
             "proposal_draw_univariate: kind must be Normal (0), Cauchy (1), Laplace (2) or Poisson (3)");
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_s;
    double *d_d, *d_u = nullptr;
    BA_TRY(st.in(scale, (size_t)nparams, &d_s));
    BA_TRY(st.out(delta, (size_t)C * nparams, &d_d));
    if (log_u) {
        BA_TRY(st.out(log_u, (size_t)C, &d_u));
    }
    BA_TRY(launch_philox_univariate(ctx, d_d, C, nparams, kind, d_s, seed, step, (uint64_t)first_chain));
    if (d_u) BA_TRY(launch_philox_chain(ctx, C, seed, step, (uint64_t)first_chain, 0, d_u, nullptr));
    BA_TRY(launch_step_advance(ctx));
    return st.finish();
}

int beatamd_gather_rows(beatamd_ctx *ctx, int64_t nout, int64_t ncols, const double *src,
                        int64_t nrows_src, const int32_t *indexes, double *out)
{
    ENTER(ctx);
    BA_CHECK(src && indexes && out && nout >= 0 && ncols > 0 && nrows_src > 0, BEATAMD_EINVAL,
             "gather_rows: bad argument");
    if (nout == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_s;
    const int32_t *d_i;
    double *d_o;
    BA_TRY(st.in(src, (size_t)nrows_src * ncols, &d_s));
    BA_TRY(st.in(indexes, (size_t)nout, &d_i));
    BA_TRY(st.out(out, (size_t)nout * ncols, &d_o));
    BA_CHECK(d_o != d_s, BEATAMD_EINVAL, "gather_rows: out must not alias src");
    BA_TRY(launch_gather_rows(ctx, nout, ncols, d_s, ncols, nrows_src, d_i, d_o, ncols));
    return st.finish();
}

// ------------------------------------------------------------------ a Metropolis step in pieces (target-sharded models)
int beatamd_like_assemble(beatamd_ctx *ctx, int64_t C, int64_t nllk, int64_t nsrc, const double *gathered,
                          const int32_t *dst_col, const double *local_ll, int64_t local_ld, int64_t local_col0,
                          int64_t n_rest, int64_t rest_dst0, int32_t ngroups, const int32_t *group_end, double *LL)
{
    ENTER(ctx);
    BA_CHECK(gathered && dst_col && LL && group_end && C >= 0 && nsrc > 0 && nllk > 1 && ngroups >= 1 && ngroups <= 8 &&
             n_rest >= 0 && (n_rest == 0 || local_ll), BEATAMD_EINVAL, "like_assemble: bad argument");
    BA_CHECK(is_device_ptr(gathered) && is_device_ptr(LL) && (!local_ll || is_device_ptr(local_ll)), BEATAMD_EINVAL,
             "like_assemble: the gathered block, the local vectors and LL live on the device");
    if (C == 0) return BEATAMD_OK;
    LikeGroups grp;
    grp.n = ngroups;
    for (int g = 0; g < ngroups; g++) {
        BA_CHECK(group_end[g] > 0 && group_end[g] < nllk && (g == 0 || group_end[g] >= group_end[g - 1]), BEATAMD_EINVAL,
                 "like_assemble: composite boundaries must ascend inside the vector");
        grp.end[g] = group_end[g];
    }
    for (int64_t r = 0; r < nsrc; r++)
        BA_CHECK(dst_col[r] >= -1 && dst_col[r] < nllk - 1, BEATAMD_EINVAL, "like_assemble: column %d of row %lld", dst_col[r], (long long)r);
    BA_CHECK(rest_dst0 >= 0 && rest_dst0 + n_rest <= nllk - 1, BEATAMD_EINVAL, "like_assemble: replicated columns outside the vector");
    Staging st(ctx);
    const int32_t *d_dc;
    BA_TRY(st.in(dst_col, (size_t)nsrc, &d_dc));
    BA_TRY(launch_like_assemble(ctx, C, nllk, nsrc, gathered, d_dc, local_ll, local_ld, local_col0, n_rest,
                                rest_dst0, grp, LL, nullptr));
    return BEATAMD_OK;
}

int beatamd_metropolis_propose(beatamd_ctx *ctx, int64_t C, int64_t nparams, const double *Q0, const double *delta,
                               const double *scaling, const double *lower, const double *upper, double *Qprop,
                               int32_t *inbounds)
{
    ENTER(ctx);
    BA_CHECK(Q0 && delta && scaling && lower && upper && Qprop && inbounds && C >= 0 && nparams > 0, BEATAMD_EINVAL,
             "metropolis_propose: bad argument");
    BA_CHECK(is_device_ptr(Q0) && is_device_ptr(delta) && is_device_ptr(scaling) && is_device_ptr(lower) && is_device_ptr(upper) &&
             is_device_ptr(Qprop) && is_device_ptr(inbounds), BEATAMD_EINVAL, "metropolis_propose: device pointers only");
    return launch_propose(ctx, C, nparams, Q0, delta, scaling, lower, upper, Qprop, inbounds);
}

int beatamd_metropolis_accept(beatamd_ctx *ctx, int64_t C, int64_t nparams, int64_t nllk, double *Q0, double *L0,
                              const double *Qprop, double *Lprop, const int32_t *inbounds, const double *log_u, double beta,
                              const double *betas, int32_t *accepted)
{
    ENTER(ctx);
    BA_CHECK(Q0 && L0 && Qprop && Lprop && inbounds && log_u && accepted && C >= 0 && nparams > 0 && nllk > 0, BEATAMD_EINVAL,
             "metropolis_accept: bad argument");
    BA_CHECK(is_device_ptr(Q0) && is_device_ptr(L0) && is_device_ptr(Qprop) && is_device_ptr(Lprop) && is_device_ptr(inbounds) &&
             is_device_ptr(log_u) && is_device_ptr(accepted) && (!betas || is_device_ptr(betas)), BEATAMD_EINVAL,
             "metropolis_accept: device pointers only");
    return launch_accept(ctx, C, nparams, nllk, Q0, L0, Qprop, Lprop, inbounds, log_u, beta, betas, accepted, nullptr, nullptr,
                         nullptr, nullptr, false);
}

int beatamd_metropolis_tune(beatamd_ctx *ctx, int64_t C, double *scaling, int32_t *accepted,
                            int32_t tune_interval)
{
    ENTER(ctx);
    BA_CHECK(scaling && accepted && C >= 0 && tune_interval > 0, BEATAMD_EINVAL,
             "metropolis_tune: bad argument");
    if (C == 0) return BEATAMD_OK;
    Staging st(ctx);
    double *d_s;
    int32_t *d_a;
    BA_TRY(st.out(scaling, (size_t)C, &d_s, true));
    BA_TRY(st.out(accepted, (size_t)C, &d_a, true));
    BA_TRY(launch_tune_scaling(ctx, C, d_s, d_a, (double)tune_interval));
    return st.finish();
}

// ------------------------------------------------------------------ whitening operator
int beatamd_chol_inverse_batch(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *covs, double *W,
                               double *log_pdet)
{
    ENTER(ctx);
    BA_CHECK(covs && W && log_pdet && nd >= 0 && n > 0, BEATAMD_EINVAL, "chol_inverse_batch: bad argument");
    if (nd == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_c;
    double *d_w, *d_l;
    BA_TRY(st.in(covs, (size_t)nd * n * n, &d_c));
    BA_TRY(st.out(W, (size_t)nd * n * n, &d_w));
    BA_TRY(st.out(log_pdet, (size_t)nd, &d_l));
    BA_TRY(launch_chol_inverse(ctx, nd, n, d_c, d_w, d_l));
    BA_TRY(ctx->check_status());
    return st.finish();
}

int beatamd_chol_inverse_batch_flags(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *covs, double *W,
                                     double *log_pdet, int32_t *not_psd)
{
    ENTER(ctx);
    BA_CHECK(covs && W && log_pdet && not_psd && nd >= 0 && n > 0, BEATAMD_EINVAL,
             "chol_inverse_batch_flags: bad argument");
    if (nd == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_c;
    double *d_w, *d_l;
    int32_t *d_f;
    BA_TRY(st.in(covs, (size_t)nd * n * n, &d_c));
    BA_TRY(st.out(W, (size_t)nd * n * n, &d_w));
    BA_TRY(st.out(log_pdet, (size_t)nd, &d_l));
    BA_TRY(st.out(not_psd, (size_t)nd, &d_f));
    BA_TRY(launch_chol_inverse(ctx, nd, n, d_c, d_w, d_l, d_f));
    return st.finish();
}

int beatamd_factor_compact(beatamd_ctx *ctx, int64_t K, int64_t n, const double *factor, double *R)
{
    ENTER(ctx);
    BA_CHECK(factor && R && K > 0 && n > 0, BEATAMD_EINVAL, "factor_compact: bad argument");
    Staging st(ctx);
    const double *d_f;
    double *d_r;
    BA_TRY(st.in(factor, (size_t)K * n, &d_f));
    BA_TRY(st.out(R, (size_t)n * n, &d_r));
    BA_TRY(launch_gram_cholesky(ctx, K, n, d_f, d_r));
    BA_TRY(ctx->check_status());
    return st.finish();
}

int beatamd_whitening_ratio_batch(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *W_new,
                                  const double *W_old, double *M)
{
    ENTER(ctx);
    BA_CHECK(W_new && W_old && M && nd >= 0 && n > 0, BEATAMD_EINVAL, "whitening_ratio_batch: bad argument");
    if (nd == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_n, *d_o;
    double *d_m;
    BA_TRY(st.in(W_new, (size_t)nd * n * n, &d_n));
    BA_TRY(st.in(W_old, (size_t)nd * n * n, &d_o));
    BA_TRY(st.out(M, (size_t)nd * n * n, &d_m));
    BA_TRY(launch_triu_ratio(ctx, nd, n, d_n, d_o, d_m));
    BA_TRY(ctx->check_status());
    return st.finish();
}

int beatamd_unwhiten_traces(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *W, double *X)
{
    ENTER(ctx);
    BA_CHECK(W && X && nd >= 0 && n > 0, BEATAMD_EINVAL, "unwhiten_traces: bad argument");
    if (nd == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_w;
    double *d_o;
    BA_TRY(st.in(W, (size_t)nd * n * n, &d_w));
    BA_TRY(st.out(X, (size_t)nd * n, &d_o, true));   // in place: host traces go up first
    BA_TRY(launch_triu_solve_vec(ctx, nd, n, d_w, d_o));
    BA_TRY(ctx->check_status());
    return st.finish();
}

int beatamd_ffi_model_update_data(beatamd_ctx *ctx, int32_t model_id, int32_t wavemap_index, const double *data)
{
    ENTER(ctx);
    FfiModel *m;
    BA_TRY(find_model(ctx, model_id, &m));
    BA_CHECK(data && wavemap_index >= 0 && (size_t)wavemap_index < m->wavemaps.size(), BEATAMD_EINVAL,
             "model_update_data: bad argument");
    Wavemap &w = m->wavemaps[wavemap_index];
    m->lsq_blocks_valid = false;
    m->obs_quads_valid = false;
    // (a spectrum wavemap's observed side is its [T,M] amplitude spectra)
    double *dst = w.domain == BEATAMD_DOMAIN_SPECTRUM ? w.data_spec.get() : w.data.get();
    BA_HIP(hipMemcpyAsync(dst, data, (size_t)w.T * w.nsamples() * 8, hipMemcpyDefault, ctx->stream));
    BA_HIP(hipStreamSynchronize(ctx->stream));
    return BEATAMD_OK;
}

// ------------------------------------------------------------------ library whitening
int beatamd_whiten_rows(beatamd_ctx *ctx, double *rows, int64_t nrows, int64_t N, const double *W)
{
    ENTER(ctx);
    BA_CHECK(rows && W && nrows >= 0 && N > 0, BEATAMD_EINVAL, "whiten_rows: bad argument");
    BA_CHECK(is_device_ptr(rows), BEATAMD_EINVAL, "whiten_rows: rows must live in HBM");
    if (nrows == 0) return BEATAMD_OK;
    drop_f32_overlapping(ctx, rows, (size_t)nrows * N * 8);
    drop_obs_quads(ctx);
    Staging st(ctx);
    const double *d_w;
    double *tmp;
    int upper = 0;
    BA_TRY(st.in(W, (size_t)N * N, &d_w));
    BA_TRY(upper_tri_flag(ctx, d_w, 1, N, &upper));
    // out-of-place per chunk (every column block of a chunk reads all of its rows), then copied back
    int64_t chunk = std::max<int64_t>(64, ((int64_t)1 << 28) / (N * 8));
    chunk = std::min(chunk, nrows);
    BA_TRY(ctx->scratch(SL_WHITEN, (size_t)chunk * N, &tmp));
    for (int64_t r0 = 0; r0 < nrows; r0 += chunk) {
        const int64_t nr = std::min(chunk, nrows - r0);
        GemmCall g;
        g.A = rows + r0 * N; g.lda = N;
        g.B = d_w; g.ldb = N; g.b_kn = 0; g.b_upper = upper;
        g.O = tmp; g.ldo = N;
        g.M = nr; g.N = N; g.K = N;
        g.timer = "whiten";
        BA_TRY(launch_gemm_f64(ctx, g));
        BA_HIP(hipMemcpyAsync(rows + r0 * N, tmp, (size_t)nr * N * 8, hipMemcpyDeviceToDevice,
                              ctx->stream));
    }
    return BEATAMD_OK;
}

// All datasets of a wavemap at once, IN PLACE and without a second buffer: with upper-triangular operators
// (chol_inverse, heart.py:233) the product column n of a row needs the row's entries k >= n only, so the columns
// are produced 128 at a time in ascending order, each launch covering that column block of every row of every
// dataset (grid.y = dataset): what a block overwrites is never read by a later launch.  No chunk buffer, no
// copy back, no triangular load imbalance inside a launch, one host synchronisation (the triangularity check).
int beatamd_whiten_rows_batch(beatamd_ctx *ctx, double *rows, int64_t nbatch, int64_t nrows, int64_t N,
                              const double *W)
{
    ENTER(ctx);
    BA_CHECK(rows && W && nbatch >= 0 && nrows >= 0 && N > 0, BEATAMD_EINVAL, "whiten_rows_batch: bad argument");
    BA_CHECK(is_device_ptr(rows), BEATAMD_EINVAL, "whiten_rows_batch: rows must live in HBM");
    BA_CHECK(nbatch <= 65535, BEATAMD_EINVAL, "whiten_rows_batch: at most 65535 datasets per call");
    if (nrows == 0 || nbatch == 0) return BEATAMD_OK;
    drop_f32_overlapping(ctx, rows, (size_t)nbatch * nrows * N * 8);
    drop_obs_quads(ctx);
    Staging st(ctx);
    const double *d_w;
    int upper = 0;
    BA_TRY(st.in(W, (size_t)nbatch * N * N, &d_w));
    BA_TRY(upper_tri_flag(ctx, d_w, nbatch, N, &upper));
    if (!upper) {
        // general operators (a QR-fallback chol_inverse, heart.py:234-237): dataset by dataset through a buffer
        for (int64_t b = 0; b < nbatch; b++)
            BA_TRY(beatamd_whiten_rows(ctx, rows + b * nrows * N, nrows, N, d_w + b * N * N));
        return BEATAMD_OK;
    }
    const int ncb = (int)((N + 127) / 128);
    for (int cb = 0; cb < ncb; cb++) {
        GemmCall g;
        g.A = rows; g.lda = N; g.sA = nrows * N;
        g.B = d_w; g.ldb = N; g.sB = N * N; g.b_kn = 0; g.b_upper = 1;
        g.O = rows; g.ldo = N; g.sO = nrows * N;
        g.M = nrows; g.N = N; g.K = N;
        g.nbatch = (int)nbatch;
        g.col_block = cb;
        g.timer = "whiten";
        BA_TRY(launch_gemm_f64(ctx, g));
    }
    return BEATAMD_OK;
}

// ------------------------------------------------------------------ half-space synthetics
int beatamd_halfspace_displacements_batch(beatamd_ctx *ctx, int64_t C, int32_t nsrc,
                                          const int32_t *kind, const double *params, int64_t nobs,
                                          const double *east, const double *north, double nu,
                                          double *out)
{
    ENTER(ctx);
    BA_CHECK(kind && params && east && north && out && C >= 0 && nsrc > 0 && nobs > 0, BEATAMD_EINVAL,
             "halfspace_displacements: bad argument");
    BA_CHECK(nu > -1.0 && nu < 0.5, BEATAMD_EINVAL, "Poisson ratio outside (-1, 0.5)");
    BA_CHECK(!is_device_ptr(kind), BEATAMD_EINVAL, "halfspace_displacements: kind must be a host array");
    for (int i = 0; i < nsrc; i++)
        BA_CHECK(kind[i] == 0 || kind[i] == 1, BEATAMD_EINVAL, "unknown source kind %d", kind[i]);
    if (C == 0) return BEATAMD_OK;
    std::vector<int64_t> poff((size_t)nsrc * 10);
    for (size_t i = 0; i < poff.size(); i++) poff[i] = (int64_t)i;
    Staging st(ctx);
    const double *d_p, *d_e, *d_n;
    const int32_t *d_k;
    const int64_t *d_o;
    double *d_out;
    BA_TRY(st.in(kind, (size_t)nsrc, &d_k));
    BA_TRY(st.in(poff.data(), poff.size(), &d_o));
    BA_TRY(st.in(params, (size_t)C * nsrc * 10, &d_p));
    BA_TRY(st.in(east, (size_t)nobs, &d_e));
    BA_TRY(st.in(north, (size_t)nobs, &d_n));
    BA_TRY(st.out(out, (size_t)C * nsrc * nobs * 3, &d_out));
    BA_TRY(launch_geom_disp(ctx, nsrc, d_k, d_o, d_p, C, nobs, d_e, d_n, nu, d_out));
    BA_TRY(st.finish());
    BA_HIP(hipStreamSynchronize(ctx->stream));   // `poff` is a stack temporary
    return BEATAMD_OK;
}

// ------------------------------------------------------------------ geodetic FFI library, fault discretization
int beatamd_geo_gf_library(beatamd_ctx *ctx, int64_t nrows, const double *params, int64_t nobs, const double *east,
                           const double *north, const double *los, const double *odw, double nu, double *G)
{
    ENTER(ctx);
    BA_CHECK(params && east && north && los && odw && G && nrows >= 0 && nobs > 0, BEATAMD_EINVAL,
             "geo_gf_library: bad argument");
    BA_CHECK(nu > -1.0 && nu < 0.5, BEATAMD_EINVAL, "Poisson ratio outside (-1, 0.5)");
    if (nrows == 0) return BEATAMD_OK;
    const int32_t kind = 0;
    int64_t poff[10];
    for (int i = 0; i < 10; i++) poff[i] = i;
    Staging st(ctx);
    const double *d_p, *d_e, *d_n, *d_l, *d_w;
    const int32_t *d_k;
    const int64_t *d_o;
    double *d_g;
    BA_TRY(st.in(&kind, (size_t)1, &d_k));
    BA_TRY(st.in(poff, (size_t)10, &d_o));
    BA_TRY(st.in(params, (size_t)nrows * 10, &d_p));
    BA_TRY(st.in(east, (size_t)nobs, &d_e));
    BA_TRY(st.in(north, (size_t)nobs, &d_n));
    BA_TRY(st.in(los, (size_t)nobs * 3, &d_l));
    BA_TRY(st.in(odw, (size_t)nobs, &d_w));
    BA_TRY(st.out(G, (size_t)nrows * nobs, &d_g));
    BA_TRY(launch_geo_gf_library(ctx, nrows, d_p, d_k, d_o, nobs, d_e, d_n, d_l, d_w, nu, d_g));
    BA_TRY(st.finish());
    BA_HIP(hipStreamSynchronize(ctx->stream));   // `kind`, `poff` are stack temporaries
    return BEATAMD_OK;
}

int beatamd_smoothing_correlated(beatamd_ctx *ctx, int64_t P, const double *coords, int32_t kind, double *L)
{
    ENTER(ctx);
    BA_CHECK(coords && L && P >= 0 && P <= 32768, BEATAMD_EINVAL, "smoothing_correlated: bad argument");
    BA_CHECK(kind == 0 || kind == 1, BEATAMD_EINVAL,
             "Resolution based discretization does not support \"nearest_neighbor\" correlation function!");
    if (P == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_c;
    double *d_l;
    BA_TRY(st.in(coords, (size_t)P * 3, &d_c));
    BA_TRY(st.out(L, (size_t)P * P, &d_l));
    BA_TRY(launch_smoothing_correlated(ctx, P, d_c, kind, d_l));
    return st.finish();
}

int beatamd_model_resolution(beatamd_ctx *ctx, int64_t P, int64_t nobs, const double *gfs, const double *L,
                             double epsilon, double *R, double *diag)
{
    ENTER(ctx);
    BA_CHECK(gfs && L && R && diag && P >= 0 && nobs > 0, BEATAMD_EINVAL, "model_resolution: bad argument");
    if (P == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_g, *d_l;
    double *d_r, *d_d;
    BA_TRY(st.in(gfs, (size_t)P * nobs, &d_g));
    BA_TRY(st.in(L, (size_t)P * P, &d_l));
    BA_TRY(st.out(R, (size_t)P * P, &d_r));
    BA_TRY(st.out(diag, (size_t)P, &d_d));
    BA_TRY(launch_model_resolution(ctx, P, nobs, d_g, d_l, epsilon, d_r, d_d));
    BA_TRY(st.finish());
    return ctx->check_status();   // a factorisation that failed raises, whichever side the outputs live on
}

int beatamd_division_rating(beatamd_ctx *ctx, int64_t P, int64_t nobs, const double *widths, const double *lengths,
                            const double *centers, const double *bottom_depth, double depth_penalty,
                            const double *data_en, const double *mean_R, double *rating, double *dmin)
{
    ENTER(ctx);
    BA_CHECK(widths && lengths && centers && bottom_depth && data_en && mean_R && rating && P >= 0 && nobs > 0,
             BEATAMD_EINVAL, "division_rating: bad argument");
    if (P == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_w, *d_l, *d_c, *d_b, *d_e, *d_m;
    double *d_r, *d_min;
    BA_TRY(st.in(widths, (size_t)P, &d_w));
    BA_TRY(st.in(lengths, (size_t)P, &d_l));
    BA_TRY(st.in(centers, (size_t)P * 3, &d_c));
    BA_TRY(st.in(bottom_depth, (size_t)P, &d_b));
    BA_TRY(st.in(data_en, (size_t)nobs * 2, &d_e));
    BA_TRY(st.in(mean_R, (size_t)P, &d_m));
    BA_TRY(st.out(rating, (size_t)P, &d_r));
    if (dmin) BA_TRY(st.out(dmin, (size_t)P, &d_min));
    else BA_TRY(ctx->scratch(SL_RATE_DMIN, (size_t)P, &d_min));
    BA_TRY(launch_division_rating(ctx, P, nobs, d_w, d_l, d_c, d_b, depth_penalty, d_e, d_m, d_min, d_r));
    return st.finish();
}

// ------------------------------------------------------------------ posterior marginals (marginals.hip)
// the K column indices idx (either side) of a population of V columns on the host, each in [0, V)
static int mg_columns(beatamd_ctx *ctx, const char *who, const int64_t *idx, int64_t K, int64_t V, std::vector<int64_t> &h)
{
    BA_TRY(host_copy(ctx, idx, (size_t)K, h));
    for (int64_t k = 0; k < K; k++)
        BA_CHECK(h[k] >= 0 && h[k] < V, BEATAMD_EINDEX, "%s: column %lld outside a population of %lld columns", who,
                 (long long)h[k], (long long)V);
    return BEATAMD_OK;
}

// BEATAMD_ENAN naming the first of the K columns d_cols (device; h_cols the same on the host) with a non-finite sample
static int mg_finite(beatamd_ctx *ctx, const char *who, const double *d_X, int64_t n, int64_t V, const int64_t *d_cols,
                     const std::vector<int64_t> &h_cols, int64_t *bad_col)
{
    const int64_t K = (int64_t)h_cols.size();
    if (bad_col) *bad_col = -1;
    if (K == 0 || n == 0) return BEATAMD_OK;
    int32_t *d_flags;
    BA_TRY(ctx->scratch(SL_MG_FLAG, (size_t)K, &d_flags));
    BA_TRY(launch_col_check(ctx, d_X, n, V, d_cols, K, d_flags));
    std::vector<int32_t> f;
    BA_TRY(host_copy(ctx, (const int32_t *)d_flags, (size_t)K, f));
    for (int64_t k = 0; k < K; k++)
        if (f[k]) {
            if (bad_col) *bad_col = h_cols[k];
            BA_CHECK(false, BEATAMD_ENAN, "%s: column %lld holds a non-finite sample", who, (long long)h_cols[k]);
        }
    return BEATAMD_OK;
}

int beatamd_column_sort(beatamd_ctx *ctx, int64_t n, int64_t V, const double *X, int64_t K, const int64_t *cols,
                        double *sorted, int64_t *bad_col)
{
    ENTER(ctx);
    BA_CHECK(n >= 1 && V >= 1 && K >= 0 && X && sorted && (cols || K == 0), BEATAMD_EINVAL, "column_sort: bad argument");
    BA_CHECK(n <= MG_SORT_MAX_N, BEATAMD_EINVAL, "column_sort: %lld samples, at most %lld", (long long)n,
             (long long)MG_SORT_MAX_N);
    std::vector<int64_t> hc;
    BA_TRY(mg_columns(ctx, "column_sort", cols, K, V, hc));
    if (K == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_X;
    const int64_t *d_c;
    double *d_s;
    BA_TRY(st.in(X, (size_t)n * V, &d_X));
    BA_TRY(st.in(cols, (size_t)K, &d_c));
    BA_TRY(mg_finite(ctx, "column_sort", d_X, n, V, d_c, hc, bad_col));
    BA_TRY(st.out(sorted, (size_t)K * n, &d_s));
    BA_TRY(launch_col_sort(ctx, d_X, n, V, d_c, K, d_s));
    return st.finish();
}

int beatamd_column_percentiles(beatamd_ctx *ctx, int64_t K, int64_t n, const double *sorted, int64_t Q, const double *q,
                               double *out)
{
    ENTER(ctx);
    BA_CHECK(K >= 0 && n >= 1 && Q >= 0 && sorted && out && (q || Q == 0), BEATAMD_EINVAL, "column_percentiles: bad argument");
    std::vector<double> hq;
    BA_TRY(host_copy(ctx, q, (size_t)Q, hq));
    for (int64_t i = 0; i < Q; i++)
        BA_CHECK(hq[i] >= 0.0 && hq[i] <= 100.0, BEATAMD_EINVAL, "Percentiles must be in the range [0, 100]");
    if (K * Q == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_s, *d_q;
    double *d_o;
    BA_TRY(st.in(sorted, (size_t)K * n, &d_s));
    BA_TRY(st.in(q, (size_t)Q, &d_q));
    BA_TRY(st.out(out, (size_t)K * Q, &d_o));
    BA_TRY(launch_col_percentiles(ctx, d_s, K, n, d_q, Q, d_o));
    return st.finish();
}

// every row of edges [R, m + 1] finite and non-decreasing (numpy: "bins must increase monotonically")
static int mg_edges(beatamd_ctx *ctx, const char *who, const double *edges, int64_t R, int64_t m)
{
    std::vector<double> h;
    BA_TRY(host_copy(ctx, edges, (size_t)(R * (m + 1)), h));
    for (int64_t r = 0; r < R; r++)
        for (int64_t i = 0; i <= m; i++) {
            const double e = h[r * (m + 1) + i];
            BA_CHECK(std::isfinite(e) && (i == 0 || e >= h[r * (m + 1) + i - 1]), BEATAMD_EINVAL,
                     "%s: the edges of row %lld must be finite and increase monotonically", who, (long long)r);
        }
    return BEATAMD_OK;
}

int beatamd_column_histograms(beatamd_ctx *ctx, int64_t K, int64_t n, const double *sorted, int64_t nb, const double *edges,
                              int64_t *counts)
{
    ENTER(ctx);
    BA_CHECK(K >= 0 && n >= 1 && nb >= 1 && sorted && edges && counts, BEATAMD_EINVAL, "column_histograms: bad argument");
    BA_TRY(mg_edges(ctx, "column_histograms", edges, K, nb));
    if (K == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_s, *d_e;
    int64_t *d_c;
    BA_TRY(st.in(sorted, (size_t)K * n, &d_s));
    BA_TRY(st.in(edges, (size_t)K * (nb + 1), &d_e));
    BA_TRY(st.out(counts, (size_t)K * nb, &d_c));
    BA_TRY(launch_col_hist(ctx, d_s, K, n, d_e, nb, d_c));
    return st.finish();
}

int beatamd_pair_hist2d(beatamd_ctx *ctx, int64_t n, int64_t V, const double *X, int64_t P, const int64_t *pairs, int32_t bx,
                        int32_t by, const double *xedges, const double *yedges, int64_t *counts, int64_t *bad_col)
{
    ENTER(ctx);
    BA_CHECK(n >= 1 && V >= 1 && P >= 0 && X && counts && xedges && yedges && (pairs || P == 0), BEATAMD_EINVAL,
             "pair_hist2d: bad argument");
    BA_CHECK(bx >= 1 && by >= 1 && bx <= MG_HIST2D_MAX_SIDE && by <= MG_HIST2D_MAX_SIDE &&
                 (int64_t)bx * by <= MG_HIST2D_MAX_CELLS,
             BEATAMD_EINVAL, "pair_hist2d: a grid of %d x %d bins; at most %d cells (128 x 128) and %d bins a side", bx, by,
             MG_HIST2D_MAX_CELLS, MG_HIST2D_MAX_SIDE);
    std::vector<int64_t> hp;
    BA_TRY(mg_columns(ctx, "pair_hist2d", pairs, 2 * P, V, hp));
    BA_TRY(mg_edges(ctx, "pair_hist2d", xedges, P, bx));
    BA_TRY(mg_edges(ctx, "pair_hist2d", yedges, P, by));
    if (P == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_X, *d_ex, *d_ey;
    const int64_t *d_p;
    int64_t *d_c;
    BA_TRY(st.in(X, (size_t)n * V, &d_X));
    BA_TRY(st.in(pairs, (size_t)2 * P, &d_p));
    BA_TRY(st.in(xedges, (size_t)P * (bx + 1), &d_ex));
    BA_TRY(st.in(yedges, (size_t)P * (by + 1), &d_ey));
    BA_TRY(mg_finite(ctx, "pair_hist2d", d_X, n, V, d_p, hp, bad_col));
    BA_TRY(st.out(counts, (size_t)P * bx * by, &d_c));
    BA_TRY(launch_pair_hist2d(ctx, d_X, n, V, d_p, P, bx, by, d_ex, d_ey, d_c));
    return st.finish();
}

// numpy.linspace(a, b, m): i * step + a, the last point b itself
static void mg_linspace(double a, double b, int m, double *out)
{
    const double step = m > 1 ? (b - a) / (double)(m - 1) : 0.0;
    for (int i = 0; i < m; i++) out[i] = (double)i * step + a;
    if (m > 1) out[m - 1] = b;
}

int beatamd_pair_kde2d(beatamd_ctx *ctx, int64_t n, int64_t V, const double *X, int64_t P, const int64_t *pairs, int32_t gx,
                       int32_t gy, int32_t skip_blocks, int32_t shape, double *Z, double *extents, int32_t *flags, int64_t *bad_col)
{
    ENTER(ctx);
    BA_CHECK(n >= 1 && V >= 1 && P >= 0 && X && Z && extents && flags && (pairs || P == 0), BEATAMD_EINVAL,
             "pair_kde2d: bad argument");
    BA_CHECK(shape >= 0 && shape <= 2, BEATAMD_EINVAL, "pair_kde2d: launch shape %d (0 chosen here, 1 wide, 2 narrow)", shape);
    BA_CHECK(gx >= 1 && gy >= 1 && (int64_t)gx * gy <= ((int64_t)1 << 24), BEATAMD_EINVAL,
             "pair_kde2d: a grid of %d x %d points; at most 2^24", gx, gy);
    std::vector<int64_t> hp;
    BA_TRY(mg_columns(ctx, "pair_kde2d", pairs, 2 * P, V, hp));
    if (P == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_X;
    const int64_t *d_p;
    BA_TRY(st.in(X, (size_t)n * V, &d_X));
    BA_TRY(st.in(pairs, (size_t)2 * P, &d_p));
    BA_TRY(mg_finite(ctx, "pair_kde2d", d_X, n, V, d_p, hp, bad_col));
    // moments -> per pair the Cholesky factor of cov * n^(-1/3) (scipy.stats.gaussian_kde: Scott's factor n^(-1/6), the
    // sample covariance with bias=False, the normalisation 1 / (2 pi n sqrt(det))), the extents and the grid
    double *d_mom;
    BA_TRY(ctx->scratch(SL_MG_MOM, (size_t)P * MG_NMOM, &d_mom));
    BA_TRY(launch_pair_moments(ctx, d_X, n, V, d_p, P, d_mom));
    std::vector<double> mom;
    BA_TRY(host_copy(ctx, (const double *)d_mom, (size_t)P * MG_NMOM, mom));
    std::vector<KdePair> par((size_t)P);
    std::vector<double> grid((size_t)P * (gx + gy)), ext((size_t)P * 4);
    std::vector<int32_t> fl((size_t)P);
    const double f2 = std::pow((double)n, -1.0 / 6.0) * std::pow((double)n, -1.0 / 6.0);
    int64_t nbad = 0;
    for (int64_t p = 0; p < P; p++) {
        const double *m = &mom[p * MG_NMOM];
        KdePair &q = par[p];
        q = KdePair();
        q.mx = m[0];
        q.my = m[1];
        bool ok = n >= 3 && hp[2 * p] != hp[2 * p + 1];
        if (ok) {
            const double c11 = m[2] / (double)(n - 1) * f2, c12 = m[3] / (double)(n - 1) * f2, c22 = m[4] / (double)(n - 1) * f2;
            ok = std::isfinite(c11) && std::isfinite(c22) && std::isfinite(c12) && c11 > 0.0 && c22 > 0.0;
            if (ok) {
                q.l11 = std::sqrt(c11);
                q.l21 = c12 / q.l11;
                const double d = c22 - q.l21 * q.l21;
                // (a remainder within rounding of c22 is a column that is a multiple of the other)
                ok = d > 4.0 * 2.220446049250313e-16 * c22;
                if (ok) {
                    q.l22 = std::sqrt(d);
                    q.scale = 1.0 / (2.0 * M_PI * (double)n * (q.l11 * q.l22));
                    ok = std::isfinite(q.scale) && q.scale > 0.0;
                }
            }
        }
        q.ok = ok ? 1 : 0;
        fl[p] = ok ? 0 : 1;
        nbad += !ok;
        for (int e = 0; e < 4; e++) ext[p * 4 + e] = m[5 + e];
        mg_linspace(m[5], m[6], gx, &grid[p * (gx + gy)]);
        mg_linspace(m[7], m[8], gy, &grid[p * (gx + gy) + gx]);
    }
    KdePair *d_par;
    double *d_grid, *d_W, *d_box, *d_Z, *d_ext;
    int32_t *d_fl;
    BA_TRY(ctx->scratch(SL_MG_PAR, (size_t)P, &d_par));
    BA_TRY(ctx->scratch(SL_MG_GRID, grid.size(), &d_grid));
    BA_TRY(ctx->scratch(SL_MG_W, (size_t)P * n * 2, &d_W));
    BA_TRY(ctx->scratch(SL_MG_BOX, (size_t)P * kde_sample_blocks(n) * 4, &d_box));
    BA_HIP(hipMemcpyAsync(d_par, par.data(), par.size() * sizeof(KdePair), hipMemcpyHostToDevice, ctx->stream));
    BA_HIP(hipMemcpyAsync(d_grid, grid.data(), grid.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    BA_TRY(st.out(Z, (size_t)P * gx * gy, &d_Z));
    BA_TRY(st.out(extents, (size_t)P * 4, &d_ext));
    BA_TRY(st.out(flags, (size_t)P, &d_fl));
    BA_HIP(hipMemcpyAsync(d_ext, ext.data(), ext.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    BA_HIP(hipMemcpyAsync(d_fl, fl.data(), fl.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    BA_TRY(launch_pair_kde2d(ctx, d_X, n, V, d_p, P, d_par, d_W, d_box, d_grid, gx, gy, skip_blocks != 0, shape, d_Z));
    BA_HIP(hipStreamSynchronize(ctx->stream));   // the host vectors above have gone up
    BA_TRY(st.finish());
    BA_CHECK(nbad == 0, BEATAMD_ENOTPSD,
             "pair_kde2d: %lld of %lld pairs have a scaled covariance without a Cholesky factor (a constant column, a column "
             "paired with itself or a multiple of the other, fewer than 3 samples); their flags are set and their Z is NaN",
             (long long)nbad, (long long)P);
    return BEATAMD_OK;
}

int beatamd_unit_vector_sum(beatamd_ctx *ctx, int64_t n, const double *lats, const double *lons, int32_t transform, double *S)
{
    ENTER(ctx);
    BA_CHECK(n >= 1 && lats && lons && S, BEATAMD_EINVAL, "unit_vector_sum: bad argument");
    Staging st(ctx);
    const double *d_la, *d_lo;
    double *d_U, *d_S;
    BA_TRY(st.in(lats, (size_t)n, &d_la));
    BA_TRY(st.in(lons, (size_t)n, &d_lo));
    BA_TRY(st.out(S, 3, &d_S));
    BA_TRY(ctx->scratch(SL_MG_W, (size_t)n * 3, &d_U));
    BA_TRY(launch_sph_unit(ctx, n, d_la, d_lo, transform != 0, d_U));
    BA_TRY(launch_sph_sum(ctx, n, d_U, d_S));
    return st.finish();
}

int beatamd_spherical_kde(beatamd_ctx *ctx, int64_t n, const double *lats0, const double *lons0, int64_t m, const double *lats,
                          const double *lons, double norm, double sigma2, int32_t shape, double *kde)
{
    ENTER(ctx);
    BA_CHECK(n >= 1 && m >= 0 && lats0 && lons0 && kde && ((lats && lons) || m == 0), BEATAMD_EINVAL,
             "spherical_kde: bad argument");
    BA_CHECK(shape >= 0 && shape <= 2, BEATAMD_EINVAL, "spherical_kde: launch shape %d (0 chosen here, 1 wide, 2 narrow)", shape);
    BA_CHECK(std::isfinite(norm) && sigma2 > 0.0 && std::isfinite(sigma2), BEATAMD_EINVAL,
             "spherical_kde: sigma^2 = %g, norm = %g", sigma2, norm);
    if (m == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_la0, *d_lo0, *d_la, *d_lo;
    double *d_U0, *d_Ug, *d_k;
    BA_TRY(st.in(lats0, (size_t)n, &d_la0));
    BA_TRY(st.in(lons0, (size_t)n, &d_lo0));
    BA_TRY(st.in(lats, (size_t)m, &d_la));
    BA_TRY(st.in(lons, (size_t)m, &d_lo));
    BA_TRY(st.out(kde, (size_t)m, &d_k));
    BA_TRY(ctx->scratch(SL_MG_W, (size_t)n * 3, &d_U0));
    BA_TRY(ctx->scratch(SL_MG_GRID, (size_t)m * 3, &d_Ug));
    BA_TRY(launch_sph_unit(ctx, n, d_la0, d_lo0, 1, d_U0));
    BA_TRY(launch_sph_unit(ctx, m, d_la, d_lo, 1, d_Ug));
    BA_TRY(launch_sph_kde(ctx, n, d_U0, m, d_Ug, norm, sigma2, shape, d_k));
    return st.finish();
}

// ------------------------------------------------------------------ mechanism ensembles (mechanisms.hip)
int beatamd_mt_decompose(beatamd_ctx *ctx, int64_t n, int32_t kind, const double *X, double *evals, double *evecs,
                         double *moments, double *ratios, double *parts, double *unit, double *uv)
{
    ENTER(ctx);
    BA_CHECK(n >= 0 && (X || n == 0) && (kind == 0 || kind == 1), BEATAMD_EINVAL,
             "mt_decompose: bad argument (kind 0: tensors [n, 6], 1: strike, dip, rake [n, 3])");
    BA_CHECK(n <= MC_MAX_N, BEATAMD_EINVAL, "mt_decompose: %lld draws, at most %lld", (long long)n, (long long)MC_MAX_N);
    if (n == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_X;
    BA_TRY(st.in(X, (size_t)n * (kind == 1 ? 3 : 6), &d_X));
    uint32_t *d_bad;
    BA_TRY(ctx->scratch(SL_MC_FLAG, 1, &d_bad));
    BA_TRY(launch_mt_check(ctx, d_X, n, kind, d_bad));
    std::vector<uint32_t> bad;
    BA_TRY(host_copy(ctx, (const uint32_t *)d_bad, 1, bad));
    BA_CHECK(bad[0] == 0xffffffffu, BEATAMD_ENAN,
             kind == 1 ? "mt_decompose: row %u holds a non-finite angle"
                       : "mt_decompose: row %u is not a moment tensor (a non-finite entry, or all six zero)",
             bad[0]);
    double *d_ev, *d_vec, *d_mom, *d_rat, *d_par, *d_unit, *d_uv;
    BA_TRY(st.out(evals, (size_t)n * 3, &d_ev));
    BA_TRY(st.out(evecs, (size_t)n * 9, &d_vec));
    BA_TRY(st.out(moments, (size_t)n * MC_NPART, &d_mom));
    BA_TRY(st.out(ratios, (size_t)n * MC_NPART, &d_rat));
    BA_TRY(st.out(parts, (size_t)n * MC_NPART * 6, &d_par));
    BA_TRY(st.out(unit, (size_t)n * MC_NPART * 6, &d_unit));
    BA_TRY(st.out(uv, (size_t)n * 2, &d_uv));
    BA_TRY(launch_mt_decompose(ctx, n, kind, d_X, d_ev, d_vec, d_mom, d_rat, d_par, d_unit, d_uv));
    return st.finish();
}

int beatamd_fuzzy_amps(beatamd_ctx *ctx, int64_t n, int32_t P, const double *unit, int64_t npix, const double *rw,
                       const int64_t *pixel_index, int32_t ny, int32_t nx, int32_t mask, int32_t shape, double *amps)
{
    ENTER(ctx);
    BA_CHECK(n >= 1 && P >= 1 && P <= 65535 && unit && amps && npix >= 0 && ((rw && pixel_index) || npix == 0),
             BEATAMD_EINVAL, "fuzzy_amps: bad argument");
    BA_CHECK(n <= MC_MAX_N, BEATAMD_EINVAL, "fuzzy_amps: %lld draws, at most %lld", (long long)n, (long long)MC_MAX_N);
    BA_CHECK(ny >= 1 && nx >= 1 && ny <= MC_MAX_RES && nx <= MC_MAX_RES, BEATAMD_EINVAL,
             "fuzzy_amps: a grid of %d x %d pixels (each side 1 to %d)", ny, nx, MC_MAX_RES);
    BA_CHECK(shape >= 0 && shape <= 2, BEATAMD_EINVAL, "fuzzy_amps: launch shape %d (0 chosen here, 1 wide, 2 narrow)", shape);
    const int64_t cells = (int64_t)ny * nx;
    BA_CHECK(npix <= cells, BEATAMD_EINVAL, "fuzzy_amps: %lld pixels in a grid of %lld", (long long)npix, (long long)cells);
    std::vector<int64_t> hp;
    BA_TRY(host_copy(ctx, pixel_index, (size_t)npix, hp));
    for (int64_t j = 0; j < npix; j++)
        BA_CHECK(hp[j] >= 0 && hp[j] < cells, BEATAMD_EINDEX, "fuzzy_amps: pixel_index[%lld] = %lld outside a grid of %lld",
                 (long long)j, (long long)hp[j], (long long)cells);
    Staging st(ctx);
    const double *d_unit, *d_rw;
    const int64_t *d_pi;
    double *d_amps, *d_sum = nullptr;
    uint32_t *d_count = nullptr;
    BA_TRY(st.in(unit, (size_t)n * P * 6, &d_unit));
    BA_TRY(st.in(rw, (size_t)6 * npix, &d_rw));
    BA_TRY(st.in(pixel_index, (size_t)npix, &d_pi));
    BA_TRY(st.out(amps, (size_t)P * cells, &d_amps));
    if (mask) BA_TRY(ctx->scratch(SL_MC_COUNT, (size_t)P * npix + 1, &d_count));
    else BA_TRY(ctx->scratch(SL_MC_SUM, (size_t)P * npix + 1, &d_sum));
    BA_TRY(launch_fuzzy_amps(ctx, n, P, d_unit, npix, d_rw, d_pi, cells, mask != 0, shape, d_count, d_sum, d_amps));
    return st.finish();
}

// ------------------------------------------------------------------ seismic FFI library producer (seislib.hip)
// the cascade (ntaps, demean [nstage]; coef [nstage, 2, SL_MAX_TAPS] = b then a, either side) as the kernels take it
static int sl_stages(beatamd_ctx *ctx, const char *who, int32_t nstage, const int32_t *ntaps, const int32_t *demean,
                     const double *coef, SlStage *out)
{
    BA_CHECK(nstage >= 0 && nstage <= SL_MAX_STAGES, BEATAMD_EINVAL, "%s: %d filter stages (at most %d)", who, nstage,
             SL_MAX_STAGES);
    BA_CHECK(nstage == 0 || (ntaps && demean && coef), BEATAMD_EINVAL, "%s: bad argument", who);
    std::vector<int32_t> nt, dm;
    std::vector<double> c;
    BA_TRY(host_copy(ctx, ntaps, (size_t)nstage, nt));
    BA_TRY(host_copy(ctx, demean, (size_t)nstage, dm));
    BA_TRY(host_copy(ctx, coef, (size_t)nstage * 2 * SL_MAX_TAPS, c));
    for (int s = 0; s < nstage; s++) {
        BA_CHECK(nt[s] >= SL_MIN_TAPS && nt[s] <= SL_MAX_TAPS, BEATAMD_EINVAL, "%s: stage %d has %d taps (%d ... %d)", who, s,
                 nt[s], SL_MIN_TAPS, SL_MAX_TAPS);
        SlStage &st = out[s];
        st.ntaps = nt[s];
        st.demean = dm[s] != 0;
        for (int k = 0; k < SL_MAX_TAPS; k++) {
            st.b[k] = k < nt[s] ? c[(s * 2) * SL_MAX_TAPS + k] : 0.0;
            st.a[k] = k < nt[s] ? c[(s * 2 + 1) * SL_MAX_TAPS + k] : 0.0;
            BA_CHECK(std::isfinite(st.b[k]) && std::isfinite(st.a[k]), BEATAMD_EINVAL, "%s: stage %d has a non-finite coefficient",
                     who, s);
        }
        BA_CHECK(st.a[0] == 1.0, BEATAMD_EINVAL, "%s: stage %d is not normalised (a[0] = %g, must be 1)", who, s, st.a[0]);
    }
    return BEATAMD_OK;
}

// *ntm: the longest source-time function of the table's lengths nt [D] (either side), each in [1, ntmax]
static int sl_lengths(beatamd_ctx *ctx, const char *who, const int32_t *nt, int64_t D, int64_t ntmax, int64_t *ntm)
{
    BA_CHECK(D >= 1 && D <= 32767 && ntmax >= 1 && ntmax <= SL_NT_MAX && nt, BEATAMD_EINVAL,
             "%s: %lld durations (1 ... 32767) of at most %lld samples (1 ... %lld)", who, (long long)D, (long long)ntmax,
             (long long)SL_NT_MAX);
    std::vector<int32_t> h;
    BA_TRY(host_copy(ctx, nt, (size_t)D, h));
    *ntm = 1;
    for (int64_t d = 0; d < D; d++) {
        BA_CHECK(h[d] >= 1 && h[d] <= ntmax, BEATAMD_EINVAL, "%s: duration %lld has %d samples (1 ... %lld)", who, (long long)d,
                 h[d], (long long)ntmax);
        *ntm = std::max<int64_t>(*ntm, h[d]);
    }
    return BEATAMD_OK;
}

int beatamd_stf_table(beatamd_ctx *ctx, int64_t D, const double *durations, double deltat, int64_t ntmax, int32_t *nt, double *A)
{
    ENTER(ctx);
    BA_CHECK(D >= 0 && (D == 0 || (durations && nt && A)) && ntmax >= 1 && ntmax <= SL_NT_MAX, BEATAMD_EINVAL,
             "stf_table: bad argument");
    BA_CHECK(std::isfinite(deltat) && deltat > 0.0, BEATAMD_EINVAL, "stf_table: deltat = %g", deltat);
    if (D == 0) return BEATAMD_OK;
    std::vector<double> h;
    BA_TRY(host_copy(ctx, durations, (size_t)D, h));
    for (int64_t d = 0; d < D; d++) {
        BA_CHECK(std::isfinite(h[d]) && h[d] >= 0.0, BEATAMD_EINVAL, "stf_table: duration %lld is %g", (long long)d, h[d]);
        BA_CHECK(std::rint(h[d] / deltat) + 1.0 <= (double)ntmax, BEATAMD_EINVAL,
                 "stf_table: duration %g has %g samples at deltat %g, the table holds %lld", h[d], std::rint(h[d] / deltat) + 1.0,
                 deltat, (long long)ntmax);
    }
    Staging st(ctx);
    const double *d_dur;
    int32_t *d_nt;
    double *d_A;
    BA_TRY(st.in(durations, (size_t)D, &d_dur));
    BA_TRY(st.out(nt, (size_t)D, &d_nt));
    BA_TRY(st.out(A, (size_t)D * ntmax, &d_A));
    BA_TRY(launch_stf_table(ctx, D, d_dur, deltat, ntmax, d_nt, d_A));
    return st.finish();
}

int beatamd_trace_filter_batch(beatamd_ctx *ctx, int64_t R, int64_t L, const double *traces, int64_t D, int64_t ntmax,
                               const int32_t *nt, const double *A, int32_t nstage, const int32_t *ntaps, const int32_t *demean,
                               const double *coef, double *Y)
{
    ENTER(ctx);
    BA_CHECK(R >= 0 && L >= 1 && A && Y && (traces || R == 0), BEATAMD_EINVAL, "trace_filter_batch: bad argument");
    SlStage stages[SL_MAX_STAGES];
    BA_TRY(sl_stages(ctx, "trace_filter_batch", nstage, ntaps, demean, coef, stages));
    int64_t ntm;
    BA_TRY(sl_lengths(ctx, "trace_filter_batch", nt, D, ntmax, &ntm));
    if (R == 0) return BEATAMD_OK;
    const int64_t Lcmax = L + ntm - 1;
    Staging st(ctx);
    const double *d_x, *d_A;
    const int32_t *d_nt;
    double *d_y;
    BA_TRY(st.in(traces, (size_t)R * L, &d_x));
    BA_TRY(st.in(nt, (size_t)D, &d_nt));
    BA_TRY(st.in(A, (size_t)D * ntmax, &d_A));
    BA_TRY(st.out(Y, (size_t)R * D * Lcmax, &d_y));
    BA_TRY(launch_stf_convolve(ctx, R, 1, 0, 1, L, d_x, D, ntmax, d_nt, d_A, Lcmax, d_y));
    for (int s = 0; s < nstage; s++) BA_TRY(launch_trace_filter(ctx, R * D, D, L, ntmax, d_nt, Lcmax, stages[s], d_y));
    return st.finish();
}

int beatamd_seis_library_fill(beatamd_ctx *ctx, int64_t T, int64_t P, int64_t L, const double *responses, int64_t D, int64_t ntmax,
                              const int32_t *nt, const double *A, int32_t nstage, const int32_t *ntaps, const int32_t *demean,
                              const double *coef, int64_t S, int64_t N, const int64_t *i0, const double *w0, int64_t patch_block,
                              double *lib)
{
    ENTER(ctx);
    BA_CHECK(T >= 1 && P >= 1 && L >= 1 && S >= 1 && S <= 32767 && N >= 1 && responses && A && i0 && w0 && lib, BEATAMD_EINVAL,
             "seis_library_fill: bad argument (T, P, L, N >= 1; 1 <= S <= 32767)");
    SlStage stages[SL_MAX_STAGES];
    BA_TRY(sl_stages(ctx, "seis_library_fill", nstage, ntaps, demean, coef, stages));
    int64_t ntm;
    BA_TRY(sl_lengths(ctx, "seis_library_fill", nt, D, ntmax, &ntm));
    const int64_t Lcmax = L + ntm - 1, pb = patch_block >= 1 ? std::min(patch_block, P) : P;
    BA_CHECK((double)T * (double)P * (double)D * (double)S * (double)N < 9.0e18 / 8.0, BEATAMD_EINVAL,
             "seis_library_fill: the library is too large");
    Staging st(ctx);
    const double *d_x, *d_A, *d_w0;
    const int32_t *d_nt;
    const int64_t *d_i0;
    double *d_lib;
    BA_TRY(st.in(responses, (size_t)T * P * L, &d_x));
    BA_TRY(st.in(nt, (size_t)D, &d_nt));
    BA_TRY(st.in(A, (size_t)D * ntmax, &d_A));
    BA_TRY(st.in(i0, (size_t)T * P * S, &d_i0));
    BA_TRY(st.in(w0, (size_t)T * P * S, &d_w0));
    BA_TRY(st.out(lib, (size_t)T * P * D * S * N, &d_lib));
    // the filtered traces of one block of patches; owned here, freed when the call leaves
    DevMem<double> Y;
    const hipError_t e = Y.try_alloc((size_t)T * pb * D * Lcmax);
    BA_CHECK(e == hipSuccess, BEATAMD_ENOMEM,
             "seis_library_fill: %zu bytes for the filtered traces of %lld patches: %s (a smaller patch_block needs less)",
             (size_t)T * pb * D * Lcmax * sizeof(double), (long long)pb, hipGetErrorString(e));
    for (int64_t p0 = 0; p0 < P; p0 += pb) {
        const int64_t n = std::min(pb, P - p0);
        BA_TRY(launch_stf_convolve(ctx, T, P, p0, n, L, d_x, D, ntmax, d_nt, d_A, Lcmax, Y.get()));
        for (int s = 0; s < nstage; s++) BA_TRY(launch_trace_filter(ctx, T * n * D, D, L, ntmax, d_nt, Lcmax, stages[s], Y.get()));
        BA_TRY(launch_library_windows(ctx, T, P, p0, n, D, L, ntmax, d_nt, Lcmax, Y.get(), S, N, d_i0, d_w0, d_lib));
    }
    BA_TRY(st.finish());
    BA_HIP(hipStreamSynchronize(ctx->stream));   // Y is freed on return
    return BEATAMD_OK;
}

// ------------------------------------------------------------------ convergence summary (convergence.hip)
// what arviz.summary computes for summary.txt (apps/beat.py:1338-1363) from the result trace (backend.py:1401-1415)
int beatamd_autocov_lags_batch(beatamd_ctx *ctx, int64_t R, int64_t n, const double *Y, int64_t lag0, int64_t nlags, double *out)
{
    ENTER(ctx);
    BA_CHECK(R >= 0 && n >= 1 && lag0 >= 0 && nlags >= 0 && ((Y && out) || R == 0 || nlags == 0), BEATAMD_EINVAL,
             "autocov_lags_batch: bad argument (R, lag0, nlags >= 0; n >= 1)");
    BA_CHECK((double)R * (double)std::max(n, nlags) < 9.0e18 / 8.0, BEATAMD_EINVAL, "autocov_lags_batch: the batch is too large");
    if (R == 0 || nlags == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_Y;
    double *d_o;
    BA_TRY(st.in(Y, (size_t)R * n, &d_Y));
    BA_TRY(st.out(out, (size_t)R * nlags, &d_o));
    BA_TRY(launch_autocov_lags(ctx, R, n, d_Y, lag0, nlags, d_o));
    return st.finish();
}

int beatamd_rank_normalize(beatamd_ctx *ctx, int64_t n, const double *A, double *z, double *ranks)
{
    ENTER(ctx);
    BA_CHECK(n >= 1 && A && z, BEATAMD_EINVAL, "rank_normalize: bad argument (n >= 1)");
    BA_CHECK(n <= MG_SORT_MAX_N, BEATAMD_EINVAL, "rank_normalize: %lld values, at most %lld", (long long)n,
             (long long)MG_SORT_MAX_N);
    Staging st(ctx);
    const double *d_A;
    double *d_z, *d_r = nullptr;
    int64_t *d_c;
    BA_TRY(st.in(A, (size_t)n, &d_A));
    BA_TRY(ctx->scratch(SL_CV_OFF, (size_t)1, &d_c));
    BA_HIP(hipMemsetAsync(d_c, 0, sizeof(int64_t), ctx->stream));
    BA_TRY(mg_finite(ctx, "rank_normalize", d_A, n, 1, d_c, std::vector<int64_t>(1, 0), nullptr));
    BA_TRY(st.out(z, (size_t)n, &d_z));
    if (ranks) BA_TRY(st.out(ranks, (size_t)n, &d_r));
    BA_TRY(launch_rank_normalize(ctx, n, d_A, d_z, d_r));
    return st.finish();
}

int beatamd_convergence_summary(beatamd_ctx *ctx, int64_t C, int64_t D, int64_t V, const double *X, int64_t K,
                                const int64_t *cols, double hdi_prob, double tau_floor, int64_t var_batch, int64_t first_lags,
                                double *out, int32_t *flags, int64_t *rounds)
{
    ENTER(ctx);
    BA_CHECK(C >= 1 && D >= 1 && V >= 1 && K >= 0 && X && (K == 0 || (cols && out && flags)), BEATAMD_EINVAL,
             "convergence_summary: bad argument (C, D, V >= 1; K >= 0)");
    BA_CHECK(hdi_prob > 0.0 && hdi_prob < 1.0, BEATAMD_EINVAL, "convergence_summary: hdi_prob %g outside (0, 1)", hdi_prob);
    BA_CHECK(var_batch >= 0 && first_lags >= 2, BEATAMD_EINVAL, "convergence_summary: var_batch %lld < 0 or first_lags %lld < 2",
             (long long)var_batch, (long long)first_lags);
    BA_CHECK((double)C * (double)D <= (double)MG_SORT_MAX_N, BEATAMD_EINVAL,
             "convergence_summary: %lld x %lld samples a variable, at most %lld", (long long)C, (long long)D,
             (long long)MG_SORT_MAX_N);
    BA_CHECK((double)C * (double)D * (double)V < 9.0e18 / 8.0, BEATAMD_EINVAL, "convergence_summary: the trace is too large");
    std::vector<int64_t> hc;
    BA_TRY(mg_columns(ctx, "convergence_summary", cols, K, V, hc));
    if (rounds) *rounds = 0;
    if (K == 0) return BEATAMD_OK;
    Staging st(ctx);
    const double *d_X;
    const int64_t *d_c;
    double *d_o;
    int32_t *d_f;
    BA_TRY(st.in(X, (size_t)C * D * V, &d_X));
    BA_TRY(st.in(cols, (size_t)K, &d_c));
    BA_TRY(st.out(out, (size_t)K * CV_NCOL, &d_o));
    BA_TRY(st.out(flags, (size_t)K, &d_f));
    BA_TRY(launch_convergence_summary(ctx, C, D, V, d_X, K, d_c, hdi_prob, tau_floor, var_batch, first_lags, d_o, d_f, rounds));
    return st.finish();
}

}  // extern "C"
