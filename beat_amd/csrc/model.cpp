// model.cpp -- the model evaluator: composites of an FfiModel, its likelihood, the fused Metropolis step (host side).
#include "model.hpp"

namespace beatamd {

int wset_quad(beatamd_ctx *ctx, const WeightSet &w, int64_t C, const double *X, int64_t xs_c, int64_t xs_d, double *quad)
{
    if (w.kind == BEATAMD_W_SCALAR)
        return launch_scalar_quad(ctx, C, w.nd, w.M, X, xs_c, xs_d, w.w.get(), quad);
    // banded whitening operators (the reference's "exponential" noise structure gives bidiagonal ones): two products per
    // sample instead of a row of the dense matrix
    if (wset_banded(ctx, w))
        return launch_quadform_banded(ctx, w.wb.get(), w.band, w.M, w.nd, C, X, xs_c, xs_d, quad, w.nd);
    QuadformCall q;
    q.A = w.w.get(); q.a_stride = w.M * w.M; q.M = w.M; q.nd = w.nd; q.C = C;
    q.X = X; q.xs_c = xs_c; q.xs_d = xs_d; q.upper_tri = w.upper_tri;
    q.quad = quad; q.q_stride = w.nd;
    return launch_quadform(ctx, q);
}

int64_t model_ndata(const FfiModel &m)
{
    int64_t n = 0;
    for (auto &w : m.wavemaps) n += w.T;
    if (m.has_geo) n += (int64_t)m.geo.sizes.size();
    return n;
}

int64_t model_nterm(const FfiModel &m) { return model_ndata(m) + (m.lap >= 0 ? m.layout.nvar : 0); }

// the cached |W d|^2 of every model go when weights, data, library rows or corrections change (a weight set or a
// whitened library may serve several models: all are dropped, the next beatamd_ffi_obs_quads recomputes)
void drop_obs_quads(beatamd_ctx *ctx)
{
    for (auto &m : ctx->models)
        if (m) m->obs_quads_valid = false;
}

int model_check_layout(const FfiModel &m)
{
    const beatamd_ffi_layout &L = m.layout;
    const int64_t np = L.nparams;
    BA_CHECK(np > 0, BEATAMD_EINVAL, "layout: nparams must be positive");
    for (int v = 0; v < L.nvar; v++)
        BA_CHECK(L.slip_off[v] >= 0 && L.slip_off[v] + m.P <= np, BEATAMD_EINVAL, "layout: slip variable %d outside q", v);
    if (!m.wavemaps.empty()) {
        BA_CHECK(L.durations_off >= 0 && L.durations_off + m.P <= np, BEATAMD_EINVAL, "layout: durations outside q");
        BA_CHECK(L.velocities_off >= 0 && L.velocities_off + m.P <= np, BEATAMD_EINVAL, "layout: velocities outside q");
        BA_CHECK(L.nuc_strike_off >= 0 && L.nuc_strike_off + m.nsub <= np && L.nuc_dip_off >= 0 &&
                     L.nuc_dip_off + m.nsub <= np && L.time_off >= 0 && L.time_off + m.nsub <= np,
                 BEATAMD_EINVAL, "layout: hypocentre variables outside q");
    }
    BA_CHECK(!m.wavemaps.empty() || m.has_geo || m.has_pol || m.lap >= 0, BEATAMD_EINVAL, "model has no composite");
    return BEATAMD_OK;
}

// ------------------------------------------------------------------ composites
int stack_all(beatamd_ctx *ctx, const SeisLib &lib, int64_t C, const double *durations, const double *starttimes,
              const double *slips, int interp, double *out)
{
    GfStackCall k;
    k.libs[0] = &lib; k.nvar = 1; k.interp = interp; k.C = C;
    k.slips[0] = ChainVec{slips, lib.P, 0}; k.durations = ChainVec{durations, lib.P, 0};
    k.st.explicit_st = starttimes; k.mode = GF_STORE_SYN; k.out = out;
    return launch_gfstack(ctx, k);
}

// chains whose indices leave the library grid / the patch grid: like = NaN (rejected by the
// Metropolis step) in addition to the status word that the next synchronisation raises
int model_start_times(beatamd_ctx *ctx, const FfiModel &m, int64_t C, const double *Q, double **st0, int32_t **chain_bad)
{
    BA_TRY(ctx->scratch(SL_CHAINBAD, (size_t)C, chain_bad));
    BA_HIP(hipMemsetAsync(*chain_bad, 0, (size_t)C * sizeof(int32_t), ctx->stream));
    BA_TRY(ctx->scratch(SL_ST0, (size_t)C * m.P, st0));
    return launch_sweep_model(ctx, m, Q, C, *st0, *chain_bad);
}

int wavemap_call(beatamd_ctx *ctx, const FfiModel &m, const Wavemap &wm, int64_t C, const double *Q, const double *st0,
                 int32_t *chain_bad, GfStackCall *call)
{
    GfStackCall &k = *call;
    const int64_t np = m.layout.nparams;
    k.nvar = m.layout.nvar;
    for (int v = 0; v < k.nvar; v++) {
        k.libs[v] = get_obj(ctx->seislibs, wm.libs[v]);
        BA_CHECK(k.libs[v] && k.libs[v]->g, BEATAMD_EINVAL, "wavemap refers to a destroyed / empty GF library");
        k.slips[v] = ChainVec{Q, np, m.layout.slip_off[v]};
    }
    k.durations = ChainVec{Q, np, m.layout.durations_off};
    k.st.starttimes0 = st0;
    k.st.Q = Q;
    k.st.nparams = np;
    k.order_key[0] = ChainVec{Q, np, m.layout.nuc_strike_off};   // (scheduling hint of k_gfstack_runs)
    k.order_key[1] = ChainVec{Q, np, m.layout.nuc_dip_off};
    k.st.shift_off = wm.shift_off.get();
    k.st.nslot = wm.nslot; k.st.tslot = wm.tslot.get(); k.st.slot_shift_off = wm.slot_shift_off.get();
    k.st.chain_bad = chain_bad;
    k.interp = wm.interp;
    k.f32 = wm.f32;
    k.C = C;
    k.data = wm.data.get();
    return BEATAMD_OK;
}

// The composite's correction table as the kernels of this call get it.  With pole terms: the derived coefficients of
// the C chains are written first (k_pole_coef, on the stream ahead of the consumer) into the composite's record buffer,
// which grows with the chain count -- never inside a graph capture (the eager step in front of a capture sizes it)
int geo_pole_coefficients(beatamd_ctx *ctx, const Geodetic &g, int64_t C, const double *Q, int64_t np, GeoCorr *gc)
{
    *gc = g.corr;
    if (g.corr.npole == 0 || C == 0) return BEATAMD_OK;
    if (C > g.pole_chains) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        BA_HIP(hipStreamIsCapturing(ctx->stream, &cap));
        BA_CHECK(cap == hipStreamCaptureStatusNone, BEATAMD_EINVAL,
                 "pole coefficients: %lld chains inside a graph capture, the buffer holds %lld (run one step before the capture)",
                 (long long)C, (long long)g.pole_chains);
        BA_HIP(hipStreamSynchronize(ctx->stream));   // (kernels in flight may read the records that go)
        g.pole_chains = 0;                           // (alloc frees what was held first: nothing is held if it fails)
        BA_TRY(g.pole_coef.alloc((size_t)C * g.corr.npole * 4));
        g.pole_chains = C;
    }
    gc->pole = g.pole_coef.get();
    return launch_pole_coef(ctx, g.corr.pole_terms, g.corr.npole, Q, np, C, g.pole_coef.get());
}

int geodetic_residual(beatamd_ctx *ctx, const FfiModel &m, int64_t C, const double *Q, double *mu_out, double *res_out)
{
    const Geodetic &g = m.geo;
    const int64_t np = m.layout.nparams;
    if (!Q) {
        BA_HIP(hipMemsetAsync(mu_out, 0, (size_t)g.Nobs * sizeof(double), ctx->stream));
        return launch_geo_residual(ctx, 1, g.Nobs, g.data.get(), g.odws.get(), mu_out, res_out);   // (d - 0) * odw
    }
    if (m.geo_is_geometry) {
        if (!res_out) return launch_geom_los(ctx, m.geom, Q, np, C, mu_out);
        // synthetics, line of sight and weighted residual in one kernel
        GeoCorr gc;
        BA_TRY(geo_pole_coefficients(ctx, g, C, Q, np, &gc));
        return launch_geom_los(ctx, m.geom, Q, np, C, nullptr, g.data.get(), g.odws.get(), res_out, gc);
    }
    // every slip variable's G.T . slips in one launch (geodetic.py:1065-1070 sums them)
    const GeoLib *gls[4] = {nullptr, nullptr, nullptr, nullptr};
    ChainVec slips[4];
    BA_CHECK(m.layout.nvar <= 4, BEATAMD_EINVAL, "geodetic composite: more than 4 slip variables");
    for (int v = 0; v < m.layout.nvar; v++) {
        gls[v] = get_obj(ctx->geolibs, g.libs[v]);
        BA_CHECK(gls[v], BEATAMD_EINVAL, "geodetic composite refers to a destroyed GF library");
        slips[v] = ChainVec{Q, np, m.layout.slip_off[v]};
    }
    BA_TRY(launch_geo_stack(ctx, gls, m.layout.nvar, C, slips, 0, mu_out));
    if (!res_out) return BEATAMD_OK;
    GeoCorr gc;
    BA_TRY(geo_pole_coefficients(ctx, g, C, Q, np, &gc));
    return launch_geo_residual(ctx, C, g.Nobs, g.data.get(), g.odws.get(), mu_out, res_out, Q, np, gc);
}

int laplacian_quad(beatamd_ctx *ctx, const Laplacian &lap, int64_t C, int64_t nvar, const double *slips, double *quad)
{
    QuadformCall q;
    q.A = lap.L.get(); q.a_stride = 0; q.M = lap.P; q.nd = nvar; q.C = C;
    q.X = slips; q.xs_c = nvar * lap.P; q.xs_d = lap.P;
    q.quad = quad; q.q_stride = nvar;
    return launch_quadform(ctx, q);
}

static int geodetic_wset(beatamd_ctx *ctx, const Geodetic &g, size_t d, WeightSet **ws)
{
    *ws = get_obj(ctx->wsets, g.wsets[d]);
    BA_CHECK(*ws && (*ws)->nd == 1 && (*ws)->M == g.sizes[d], BEATAMD_EINVAL,
             "geodetic dataset %zu: weight set missing or of the wrong size", d);
    return BEATAMD_OK;
}

// the polarity composite's launch up to what its caller wants of it (mode, out, ld, active)
void polarity_call(const Polarity &p, int64_t C, const double *Q, int64_t np, PolArgs *a)
{
    a->src = p.src; a->nmap = p.nmap; a->ntab = p.ntab; a->NT = p.NT;
    for (int i = 0; i < POL_MAX_MAPS; i++) {
        a->map_end[i] = p.map_end[i]; a->hp_off[i] = p.hp_off[i]; a->hp_fix[i] = p.hp_fix[i];
    }
    a->gamma = p.gamma;
    a->rw = p.rw.get(); a->obs = p.obs.get(); a->utab = p.utab.get(); a->btab = p.btab.get();
    a->Q = Q; a->nparams = np; a->C = C;
}

// ------------------------------------------------------------------ likelihood
// With opt.llks every composite stops in front of its epilogue and stores the quadratic form it would have handed to it
// (update_llks: seismic.py:510-525, geodetic.py:429-444, laplacian.py:141-154); the hyper-parameters are then not read
int ffi_logp_device(beatamd_ctx *ctx, FfiModel &m, int64_t C, const double *Q, double *LL, const LogpOpts &opt)
{
    const int64_t nllk = m.nllk(), nterm = model_nterm(m), np = m.layout.nparams;
    double *const llks = opt.llks;
    BA_CHECK(!(llks && m.has_pol), BEATAMD_EINVAL,
             "the polarity composite has no Gaussian misfit: update_llks / variance reductions are not defined for it "
             "(beat/models/polarity.py defines none)");
    int64_t col = 0, tcol = 0;   // next column of LL / of llks
    LikeGroups grp;
    double *quad;
    WeightSet *ws;
    int32_t *chain_bad = nullptr;   // (only the seismic index maps and the sweep flag chains)

    if (!m.wavemaps.empty()) {
        double *st0;
        BA_TRY(model_start_times(ctx, m, C, Q, &st0, &chain_bad));
        for (auto &wm : m.wavemaps) {
            ws = get_obj(ctx->wsets, wm.wset);
            BA_CHECK(ws, BEATAMD_EINVAL, "wavemap refers to a destroyed weight set");
            GfStackCall k;
            BA_TRY(wavemap_call(ctx, m, wm, C, Q, st0, chain_bad, &k));
            k.active = opt.active;
            BA_TRY(ctx->scratch(SL_QUAD, (size_t)C * wm.T, &quad));
            if (wm.domain == BEATAMD_DOMAIN_SPECTRUM) {
                // the amplitude is taken after the stack, so nothing of the misfit can ride in the stacking kernel: the
                // time-domain traces go to scratch, k_amp_spectrum writes data_spec - spec(syn) once, and every weight
                // kind takes its quadratic form of that (M samples per dataset in place of N from here on)
                double *spec;
                BA_CHECK(ws->nd == wm.T && ws->M == wm.M, BEATAMD_EINVAL, "spectrum wavemap: weight set of the wrong size");
                k.mode = GF_STORE_SYN;
                BA_TRY(ctx->scratch(SL_RESID, (size_t)C * wm.T * wm.N, &k.out));
                BA_TRY(ctx->scratch(SL_SPEC, (size_t)C * wm.T * wm.M, &spec));
                BA_TRY(launch_gfstack(ctx, k));
                BA_TRY(launch_amp_spectrum(ctx, C * wm.T, wm.N, wm.N, wm.ntrans, wm.lo, wm.hi, k.out, wm.data_spec.get(), wm.T,
                                           spec));
                BA_TRY(wset_quad(ctx, *ws, C, spec, wm.T * wm.M, wm.M, quad));
            } else if (ws->kind == BEATAMD_W_SCALAR) {
                k.mode = GF_RESID_SCALAR;
                k.wscalar = ws->w.get();
                k.quad = quad;
                BA_TRY(launch_gfstack(ctx, k));
            } else if (ws->band == 1 && ws->M == wm.N && ws->nd == wm.T && wset_banded(ctx, *ws)) {
                // bidiagonal whitening operators (the "exponential" noise structure): the misfit rides in the stacking
                // kernel where it has the epilogue, else residual store + k_quadform_band1 (launch_gfstack decides)
                k.mode = GF_RESID_BAND1;
                k.band_w = ws->wb.get();
                k.quad = quad;
                BA_TRY(ctx->scratch(SL_RESID, (size_t)C * wm.T * wm.N, &k.out));
                BA_TRY(launch_gfstack(ctx, k));
            } else {
                k.mode = GF_RESID_STORE;
                BA_TRY(ctx->scratch(SL_RESID, (size_t)C * wm.T * wm.N, &k.out));
                BA_TRY(launch_gfstack(ctx, k));
                BA_TRY(wset_quad(ctx, *ws, C, k.out, wm.T * wm.N, wm.N, quad));
            }
            if (llks)
                BA_TRY(launch_store_misfits(ctx, C, wm.T, quad, llks + tcol, nterm));
            else
                BA_TRY(launch_mvn_finish(ctx, C, wm.T, wm.nsamples(), quad, ws->slog.get(), HpSrc{Q, np, wm.hp_off.get()}, LL + col,
                                         nllk));
            col += wm.T;
            tcol += wm.T;
        }
        grp.end[grp.n++] = (int32_t)col;
    }
    if (m.has_geo) {
        const Geodetic &g = m.geo;
        const size_t nd = g.sizes.size();
        double *mu;
        BA_TRY(ctx->scratch(SL_MU, (size_t)C * g.Nobs * 2, &mu));
        double *res = mu + C * g.Nobs;
        BA_TRY(geodetic_residual(ctx, m, C, Q, mu, res));
        // small dense datasets (SAR scenes / GNSS of a few hundred points): every dataset's
        // quadratic form and MVN epilogue in one launch; otherwise per dataset on the 64-row tiles
        QuadformSmallCall qs;
        bool small = nd <= 8;
        int64_t off = 0;
        for (size_t d = 0; d < nd; d++) {
            BA_TRY(geodetic_wset(ctx, g, d, &ws));
            small = small && ws->kind != BEATAMD_W_SCALAR;
            if (small) {
                qs.A[d] = ws->w.get(); qs.M[d] = ws->M; qs.xoff[d] = off; qs.upper_tri[d] = ws->upper_tri;
                qs.slog[d] = ws->slog.get(); qs.hp_off[d] = g.hp_off.get() + d;
            }
            off += g.sizes[d];
        }
        small = small && quadform_small_applicable((int)nd, qs.M);
        if (small) {
            qs.nd = (int)nd;
            qs.C = C; qs.X = res; qs.xs_c = g.Nobs; qs.Q = Q; qs.nparams = np;
            qs.LL = LL + col; qs.ld = nllk;
            if (llks) {
                qs.LL = llks + tcol; qs.ld = nterm; qs.misfit_only = true;
            }
            BA_TRY(launch_quadform_small(ctx, qs));
        } else {
            BA_TRY(ctx->scratch(SL_QUAD, (size_t)C, &quad));
            off = 0;
            for (size_t d = 0; d < nd; d++) {
                ws = get_obj(ctx->wsets, g.wsets[d]);
                BA_TRY(wset_quad(ctx, *ws, C, res + off, g.Nobs, 0, quad));
                if (llks)
                    BA_TRY(launch_store_misfits(ctx, C, 1, quad, llks + tcol + (int64_t)d, nterm));
                else
                    BA_TRY(launch_mvn_finish(ctx, C, 1, ws->M, quad, ws->slog.get(), HpSrc{Q, np, g.hp_off.get() + d},
                                             LL + col + (int64_t)d, nllk));
                off += g.sizes[d];
            }
        }
        col += (int64_t)nd;
        tcol += (int64_t)nd;
        grp.end[grp.n++] = (int32_t)col;
    }
    if (m.has_pol) {
        // polarity_like is a vector, one entry per station of every map (polarity.py:133): all maps in one launch
        PolArgs a;
        polarity_call(m.pol, C, Q, np, &a);
        a.mode = POL_OUT_LLK; a.out = LL + col; a.ld = nllk; a.active = opt.active;
        BA_TRY(launch_polarity(ctx, a));
        col += m.pol.NT;
        grp.end[grp.n++] = (int32_t)col;
    }
    if (m.lap >= 0) {
        Laplacian *lp = get_obj(ctx->laps, m.lap);
        BA_CHECK(lp, BEATAMD_EINVAL, "model refers to a destroyed laplacian");
        const int nvar = m.layout.nvar;
        ChainVec slips[4];
        for (int v = 0; v < nvar; v++) slips[v] = ChainVec{Q, np, m.layout.slip_off[v]};
        double *sl;
        BA_TRY(ctx->scratch(SL_SLIPS, (size_t)C * nvar * lp->P, &sl));
        BA_TRY(launch_gather_slips(ctx, C, nvar, lp->P, slips, sl));
        BA_TRY(ctx->scratch(SL_QUAD, (size_t)C * nvar, &quad));
        BA_TRY(laplacian_quad(ctx, *lp, C, nvar, sl, quad));
        if (llks)   // one column per slip variable: the hyper model keeps them apart (laplacian.py:151-170)
            BA_TRY(launch_store_misfits(ctx, C, nvar, quad, llks + tcol, nterm));
        else
            BA_TRY(launch_laplacian_finish(ctx, C, nvar, lp->P, lp->logdet, quad, HpSrc{Q + m.layout.h_laplacian_off, np, nullptr},
                                           LL + col, nllk));
        col += 1;
        tcol += nvar;
        grp.end[grp.n++] = (int32_t)col;
    }
    BA_CHECK(col == nllk - 1, BEATAMD_EINVAL, "internal: llk layout mismatch");
    if (llks) {
        BA_CHECK(tcol == nterm, BEATAMD_EINVAL, "internal: misfit layout mismatch");
        return launch_misfits_mark_bad(ctx, C, nterm, llks, chain_bad);
    }
    if (opt.tail) {
        opt.tail->grp = grp;
        opt.tail->chain_bad = chain_bad;
        return BEATAMD_OK;
    }
    return launch_like_sum(ctx, C, nllk, grp, LL, chain_bad);
}

int model_obs_quads(beatamd_ctx *ctx, FfiModel &m)
{
    BA_CHECK(!m.has_pol, BEATAMD_EINVAL,
             "the polarity composite has no Gaussian misfit: variance reductions are not defined for it");
    const int64_t ndata = model_ndata(m);
    if (m.obs_quads_valid && (int64_t)m.obs_quads.size() == ndata) return BEATAMD_OK;
    BA_HIP(hipStreamSynchronize(ctx->stream));   // (a kernel in flight may still read the old copy)
    DevMem<double> dq;
    BA_TRY(dq.alloc((size_t)ndata));
    int64_t col = 0;
    WeightSet *ws;
    for (auto &wm : m.wavemaps) {
        ws = get_obj(ctx->wsets, wm.wset);
        const int64_t ns = wm.nsamples();   // (a spectrum wavemap's observed side is data_spec [T,M])
        BA_CHECK(ws && ws->nd == wm.T && ws->M == ns, BEATAMD_EINVAL, "wavemap refers to a destroyed weight set");
        BA_TRY(wset_quad(ctx, *ws, 1, wm.domain == BEATAMD_DOMAIN_SPECTRUM ? wm.data_spec.get() : wm.data.get(), wm.T * ns, ns,
                         dq.get() + col));
        col += wm.T;
    }
    if (m.has_geo) {
        const Geodetic &g = m.geo;
        double *mu;
        BA_TRY(ctx->scratch(SL_MU, (size_t)g.Nobs * 2, &mu));
        double *res = mu + g.Nobs;
        BA_TRY(geodetic_residual(ctx, m, 1, nullptr, mu, res));
        int64_t off = 0;
        for (size_t d = 0; d < g.sizes.size(); d++) {
            BA_TRY(geodetic_wset(ctx, g, d, &ws));
            BA_TRY(wset_quad(ctx, *ws, 1, res + off, g.Nobs, 0, dq.get() + col + (int64_t)d));
            off += g.sizes[d];
        }
        col += (int64_t)g.sizes.size();
    }
    BA_CHECK(col == ndata, BEATAMD_EINVAL, "internal: dataset layout mismatch");
    m.obs_quads.resize((size_t)ndata);
    if (ndata > 0) {
        BA_HIP(hipMemcpyAsync(m.obs_quads.data(), dq.get(), (size_t)ndata * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        BA_HIP(hipStreamSynchronize(ctx->stream));
    }
    m.d_obs_quads = std::move(dq);
    m.obs_quads_valid = true;
    return BEATAMD_OK;
}

// ------------------------------------------------------------------ lsq start
// G_v G_v^T and L^T L, once per model, on the matrix cores (lower tiles; k_lsq_finish reads the lower triangle)
static int lsq_blocks(beatamd_ctx *ctx, FfiModel &m, const Laplacian &lp, const GeoLib *gl)
{
    if (m.lsq_blocks_valid) return BEATAMD_OK;
    const int64_t P = m.P;
    BA_TRY(m.lsq_LtL.alloc((size_t)(P * P)));
    double *Lt;
    BA_TRY(ctx->scratch(SL_LSQ_U, (size_t)(P * P), &Lt));
    BA_TRY(launch_lsq_transpose(ctx, lp.L.get(), Lt, P));
    GemmCall g;
    g.A = Lt; g.B = Lt; g.lda = P; g.ldb = P; g.O = m.lsq_LtL.get(); g.ldo = P;
    g.M = P; g.N = P; g.K = P; g.b_kn = 0; g.lower_only = 1; g.timer = "lsq_blocks";
    BA_TRY(launch_gemm_f64(ctx, g));
    m.lsq_GG.reset();
    if (gl) {
        BA_TRY(m.lsq_GG.alloc((size_t)(P * P)));
        g.A = gl->g.get(); g.B = gl->g.get(); g.lda = gl->Nobs; g.ldb = gl->Nobs; g.K = gl->Nobs; g.O = m.lsq_GG.get();
        BA_TRY(launch_gemm_f64(ctx, g));
    }
    BA_HIP(hipStreamSynchronize(ctx->stream));   // (the transposed operator lives in a scratch slot)
    m.lsq_blocks_valid = true;
    return BEATAMD_OK;
}

int lsq_normal_device(beatamd_ctx *ctx, FfiModel &m, int64_t C, const double *Q, double *Nmat, double *b, int32_t **chain_bad)
{
    const int64_t P = m.P, np = m.layout.nparams;
    BA_CHECK(m.lap >= 0, BEATAMD_EINVAL,
             "Least-squares- solution for distributed slip is only available with laplacian regularization!");
    BA_CHECK(m.lsq_var >= 0 && m.lsq_var < m.layout.nvar, BEATAMD_EINVAL,
             "lsq: the model has no inverted slip variable (beatamd_ffi_model_set_lsq_variables)");
    BA_CHECK(!(m.has_geo && m.geo_is_geometry), BEATAMD_EINVAL, "lsq: a geometry-mode geodetic composite is not linear in slip");
    BA_CHECK(!m.has_pol, BEATAMD_EINVAL, "lsq: a model with a polarity composite has no linear slip problem");
    for (auto &wm : m.wavemaps)
        BA_CHECK(wm.domain != BEATAMD_DOMAIN_SPECTRUM, BEATAMD_EINVAL,
                 "lsq: a spectrum-domain wavemap is not linear in slip (the amplitude is taken after the stack)");
    Laplacian *lp = get_obj(ctx->laps, m.lap);
    BA_CHECK(lp && lp->P == P, BEATAMD_EINVAL, "model refers to a destroyed laplacian");
    const GeoLib *gl = nullptr;
    if (m.has_geo) {
        gl = get_obj(ctx->geolibs, m.geo.libs[m.lsq_var]);
        BA_CHECK(gl && gl->P == P, BEATAMD_EINVAL, "geodetic composite refers to a destroyed GF library");
    }
    BA_TRY(lsq_blocks(ctx, m, *lp, gl));
    *chain_bad = nullptr;
    int has_seis = 0;
    if (!m.wavemaps.empty()) {
        double *st0;
        BA_TRY(model_start_times(ctx, m, C, Q, &st0, chain_bad));
        for (auto &wm : m.wavemaps) {
            GfStackCall k;
            BA_TRY(wavemap_call(ctx, m, wm, C, Q, st0, *chain_bad, &k));
            const SeisLib *lib = k.libs[m.lsq_var];
            k.libs[0] = lib;      // (the tables depend on the library's grid alone, the same for every slip variable)
            uint32_t *rowoff;
            double *fac = nullptr;
            const int nrow = wm.interp == BEATAMD_MULTILINEAR ? 4 : 1;
            BA_TRY(ctx->scratch(SL_ROWOFF, (size_t)(C * lib->T * P * nrow), &rowoff));
            if (nrow == 4) BA_TRY(ctx->scratch(SL_WEIGHTS, (size_t)(C * lib->T * P * 4), &fac));
            BA_TRY(launch_gf_tables(ctx, k, rowoff, fac));
            BA_TRY(launch_lsq_seismic(ctx, *lib, wm.interp, C, rowoff, fac, wm.data.get(), has_seis, Nmat, b));
            has_seis = 1;
        }
    }
    GeoCorr gc;
    if (m.has_geo) BA_TRY(geo_pole_coefficients(ctx, m.geo, C, Q, np, &gc));
    return launch_lsq_finish(ctx, C, P, Nmat, b, has_seis, m.lsq_GG.get(), m.lsq_LtL.get(), gl ? gl->g.get() : nullptr,
                             m.has_geo ? m.geo.Nobs : 0, m.has_geo ? m.geo.data.get() : nullptr, gc, Q, np,
                             m.layout.h_laplacian_off);
}

// ------------------------------------------------------------------ fused Metropolis step
int draw_multivariate(beatamd_ctx *ctx, int64_t C, int64_t K, int64_t np, const double *factor, int df, uint64_t seed,
                      uint32_t step, uint64_t first_chain, double *delta, double *log_u, int64_t groups)
{
    double *z, *rs = nullptr;
    BA_TRY(ctx->scratch(SL_Z, (size_t)C * K, &z));
    if (df > 0) BA_TRY(ctx->scratch(SL_ROWSCALE, (size_t)C, &rs));
    BA_TRY(launch_philox_normal(ctx, z, C, K, seed, step, first_chain));
    if (log_u || rs) BA_TRY(launch_philox_chain(ctx, C, seed, step, first_chain, df, log_u, rs));
    GemmCall g;
    g.A = z; g.lda = K;
    g.B = factor; g.ldb = np; g.b_kn = 1;
    g.O = delta; g.ldo = np;
    g.M = C; g.N = np; g.K = K;
    g.row_scale = rs;
    if (groups > 1) {   // one product per group: an entry's sum over k is the one of the single product
        const int64_t R = C / groups;
        g.M = R; g.nbatch = (int)groups;
        g.sA = R * K; g.sB = K * np; g.sO = R * np; g.sR = R;
    }
    g.timer = "proposal";
    return launch_gemm_f64(ctx, g);
}

// the proposals of a step drawn on the device: qprop, their in-box flags inb and log_u (*lu, a scratch slot)
static int draw_proposals(beatamd_ctx *ctx, const StepDraw &draw, int64_t C, int64_t np, const double *d_f, const double *d_q0,
                          const double *d_sc, const double *d_lo, const double *d_up, double *qprop, int32_t *inb,
                          const double **lu_out)
{
    const int64_t K = draw.kind < 0 ? draw.K : np;
    double *lu, *de;
    BA_TRY(ctx->scratch(SL_LOGU, (size_t)C, &lu));
    *lu_out = lu;
    if (draw_propose_applicable(K, np))
        return launch_draw_propose(ctx, C, K, np, draw.kind, d_f, draw.df, draw.seed, draw.step, draw.first_chain, d_q0, d_sc,
                                   d_lo, d_up, qprop, lu, inb, draw.groups);
    BA_TRY(ctx->scratch(SL_DELTA, (size_t)C * np, &de));
    if (draw.kind < 0) {
        BA_TRY(draw_multivariate(ctx, C, K, np, d_f, draw.df, draw.seed, draw.step, draw.first_chain, de, lu, draw.groups));
    } else {
        BA_TRY(launch_philox_univariate(ctx, de, C, np, draw.kind, d_f, draw.seed, draw.step, draw.first_chain));
        BA_TRY(launch_philox_chain(ctx, C, draw.seed, draw.step, draw.first_chain, 0, lu, nullptr));
    }
    return launch_propose(ctx, C, np, d_q0, de, d_sc, d_lo, d_up, qprop, inb);
}

int astep_impl(beatamd_ctx *ctx, FfiModel &m, int64_t C, double *Q0, double *L0, const double *delta, const double *scaling,
               const double *lower, const double *upper, const double *log_u, double beta, const double *betas,
               int32_t *accepted, const StepDraw *draw, int32_t *acc_sum, int64_t *n_acc)
{
    BA_CHECK(Q0 && L0 && scaling && lower && upper && accepted && C >= 0 && (draw || (delta && log_u)),
             BEATAMD_EINVAL, "ffi_astep: NULL argument");
    BA_TRY(model_check_layout(m));
    if (C == 0) return BEATAMD_OK;
    const int64_t np = m.layout.nparams, nllk = m.nllk();
    Staging st(ctx);
    const double *d_de = nullptr, *d_sc, *d_lo, *d_up, *d_lu = nullptr, *d_be = nullptr, *d_f = nullptr;
    double *d_q0, *d_l0, *qprop, *lprop;
    int32_t *d_acc;
    BA_TRY(st.out(Q0, (size_t)C * np, &d_q0, true));
    BA_TRY(st.out(L0, (size_t)C * nllk, &d_l0, true));
    BA_TRY(st.out(accepted, (size_t)C, &d_acc));
    BA_TRY(st.in(scaling, (size_t)C, &d_sc));
    BA_TRY(st.in(lower, (size_t)np, &d_lo));
    BA_TRY(st.in(upper, (size_t)np, &d_up));
    if (betas) BA_TRY(st.in(betas, (size_t)C, &d_be));
    BA_TRY(ctx->scratch(SL_QPROP, (size_t)C * np, &qprop));
    BA_TRY(ctx->scratch(SL_LPROP, (size_t)C * nllk, &lprop));
    void *p = nullptr;   // sized in bytes on purpose: the in-box flags and 64 bytes behind them
    BA_TRY(ctx->get_scratch(SL_MISC, (size_t)C * 4 + 64, &p));
    int32_t *inb = (int32_t *)p;
    if (draw) {
        BA_CHECK(is_device_ptr(Q0) && (!acc_sum || is_device_ptr(acc_sum)) && (!n_acc || is_device_ptr(n_acc)),
                 BEATAMD_EINVAL, "ffi_mstep: chain states and counters live on the device");
        BA_TRY(st.in(draw->factor, (size_t)(draw->kind < 0 ? draw->groups * draw->K * np : np), &d_f));
        BA_TRY(draw_proposals(ctx, *draw, C, np, d_f, d_q0, d_sc, d_lo, d_up, qprop, inb, &d_lu));
    } else {
        BA_TRY(st.in(delta, (size_t)C * np, &d_de));
        BA_TRY(st.in(log_u, (size_t)C, &d_lu));
        BA_TRY(launch_propose(ctx, C, np, d_q0, d_de, d_sc, d_lo, d_up, qprop, inb));
    }
    // the `like` sum rides in the accept kernel (one launch fewer) while the row fits its LDS stage
    LikeTail tail;
    const bool fold = nllk * 8 <= 48 * 1024;
    LogpOpts opt;
    opt.tail = fold ? &tail : nullptr;
    // proposals outside the prior box are parked on their current point and always rejected: their likelihood rows are
    // never read (k_accept), so the stacking kernel may skip them (BEATAMD_SKIP_PARKED=0: evaluate every chain)
    opt.active = GfKnobs::get(gf_knobs(ctx).skip_parked, 1) != 0 ? inb : nullptr;
    BA_TRY(ffi_logp_device(ctx, m, C, qprop, lprop, opt));
    BA_TRY(launch_accept(ctx, C, np, nllk, d_q0, d_l0, qprop, lprop, inb, d_lu, beta, d_be, d_acc,
                         fold ? &tail.grp : nullptr, tail.chain_bad, acc_sum, n_acc, draw != nullptr));
    return st.finish();
}

}  // namespace beatamd
