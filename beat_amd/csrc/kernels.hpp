// kernels.hpp -- launch interfaces of the HIP kernels (internal).
#pragma once
#include <algorithm>

#include "ctx.hpp"

namespace beatamd {

// ---- sweep.hip -------------------------------------------------------------------
// what a sweep launch asks for, by the largest subfault of the batch (a pure function; beatamd_fast_sweep_lds)
constexpr int SWEEP_MAX_CELLS = 6400;
struct SweepLdsPlan {
    int nmax;       // LDS doubles per array per wavefront
    int waves;      // grids (wavefronts) per workgroup: 4 or 1
    size_t bytes;   // dynamic LDS of a workgroup
};
SweepLdsPlan sweep_lds_plan(int nmax_cells);
int launch_sweep_explicit(beatamd_ctx *ctx, const double *slow, double h, const int32_t *hi,
                          const int32_t *hj, int ni, int nj, int64_t C, double *out);
int launch_sweep_model(beatamd_ctx *ctx, const FfiModel &m, const double *Q, int64_t C,
                       double *starttimes0, int32_t *chain_bad);

// ---- gfstack.hip -----------------------------------------------------------------
// Where the per-(chain,target,patch) start times come from.
struct StartTimeSrc {
    // explicit: st[(c*T + t)*P + p]
    const double *explicit_st = nullptr;
    // model: st = starttimes0[c*P + p] - Q[c*nparams + shift_off[t]]   (seismic.py:1283-1296)
    const double *starttimes0 = nullptr;
    const double *Q = nullptr;
    int64_t nparams = 0;
    const int64_t *shift_off = nullptr;  // device [T] or nullptr (no station corrections)
    // table slots: targets with the same shift variable share their index tables (nslot > 0: tslot [T] -> slot,
    // slot_shift_off [nslot]; device pointers)
    int32_t nslot = 0;
    const int32_t *tslot = nullptr;
    const int64_t *slot_shift_off = nullptr;
    // model mode: chains whose times fall outside the library grid are marked here (their
    // `like` becomes NaN, which the Metropolis step rejects); nullptr in the explicit API
    int32_t *chain_bad = nullptr;
};

// a strided view of per-chain vectors: value(c, k) = base[c*stride + off + k]
struct ChainVec {
    const double *base = nullptr;
    int64_t stride = 0, off = 0;
};

// Workgroup id -> work item for table kernels whose NEIGHBOURING items read the same cache lines (the [C,T,P,*] index
// tables: the entries of consecutive patches of a chain share a 128-byte line).  The hardware deals consecutive workgroup
// ids round-robin to the 8 XCDs, each with its own L2 -- eight neighbours would fetch the line eight times.  Inside every
// aligned block of 64 ids the items are dealt so that an XCD gets 8 CONSECUTIVE items (ids b = x mod 8 -> items 8x .. 8x+7).
#ifdef __HIPCC__
__device__ __forceinline__ int64_t xcd_items8(int64_t b, int64_t n)
{
    if (b >= (n & ~(int64_t)63)) return b;
    const int64_t r = b & 63;
    return (b & ~(int64_t)63) + (r & 7) * 8 + (r >> 3);
}
#endif

// patch ranges a short-trace library is stacked in (gfstack.hip; 1: as it is)
int gf_patch_ranges(int64_t T, int64_t P, int64_t N, int num_cu);

enum GfMode : int {
    GF_STORE_SYN = 0,     // out[c,t,n] = synthetics                      (stack_all)
    GF_RESID_SCALAR = 1,  // partial[c,t,tile] = sum (w_t (d - syn))^2     (fused logp, W = w I)
    GF_RESID_STORE = 2,   // out[c,t,n] = d[t,n] - synthetics              (feeds the dense W quadform)
    // bidiagonal whitening operator (the reference's "exponential" noise structure, covariance.py:24-51; band detected at
    // weights_create, quadform.hip): quad[c,t] = sum_i (w0_i r_i + w1_i r_{i+1})^2 (distributions.py:119-138 with a
    // bidiagonal W) without storing the residuals.  Kernels WITH this epilogue (k_gfstack_ws): the inner samples of a tile
    // in the kernel, the last sample of every tile -- its neighbour is the next tile's first residual -- by the tile-sum
    // kernel from two edge residuals per (chain, target, tile).  Kernels without it store the residuals (mode 2) and
    // launch_gfstack runs k_quadform_band1 behind them: either way the caller gets `quad`.
    GF_RESID_BAND1 = 3
};

struct GfStackCall {
    const SeisLib *libs[4] = {nullptr, nullptr, nullptr, nullptr};
    int nvar = 1;
    ChainVec slips[4];
    ChainVec durations;
    StartTimeSrc st;
    int interp = 0;
    int64_t C = 0;
    int mode = GF_STORE_SYN;
    const double *data = nullptr;     // [T,N]   (modes 1,2)
    const double *wscalar = nullptr;  // [T]     (mode 1)
    double *out = nullptr;            // [C,T,N] (modes 0,2)
    double *quad = nullptr;           // [C,T]   (modes 1, 3) sum over tiles, fixed order
    const double *band_w = nullptr;   // [T,N,2] (mode 3) row i of the bidiagonal operator: (W[i,i], W[i,i+1]), 0 behind the end
    bool f32 = false;                 // rows from the libraries' float copies where the kernel supports it
    // optional scheduling hint: two per-chain sort keys that put chains which rupture alike next to each other
    // (the fused model path: hypocentre strike / dip of the first subfault).  Never changes a result.
    ChainVec order_key[2];
    // optional [C] mask (the fused Metropolis step: proposals inside the prior box).  A kernel that honours it may leave the
    // outputs of chains with active[c] == 0 unwritten; one that ignores it evaluates them (their points are in the grid).
    const int32_t *active = nullptr;
};
int launch_gfstack(beatamd_ctx *ctx, const GfStackCall &call);
// quad[i] = the tiles of partial [n = C*T, ntile] joined in ascending order (k_sum_tiles, the orders of misfit.hpp); mode 3
// (edges given): with every tile's boundary term from edges [C*T, ntile, 2] = (first, last residual of the 64-sample tile)
int launch_sum_tiles(beatamd_ctx *ctx, const double *partial, int64_t n, int ntile, double *quad, const int *guard = nullptr,
                     int want = 0, const double *edges = nullptr, const double *band_w = nullptr, int64_t T = 1, int64_t N = 0);
// g[i] = (double)(float)g[i]; g32[i] = (float)g[i]  (float-storage copy of a GF library)
int launch_round_to_f32(beatamd_ctx *ctx, double *g, float *g32, int64_t n);
// ---- the plan of one stacking call: every decision taken before anything is launched, taken once (gf_plan_call, gfstack.hip,
// and its callees next to the kernels whose limits they state).  The launch functions read it and decide nothing.
// Who evaluates the bidiagonal misfit (mode 3): the combine kernel of the patch ranges (k_split_combine), the runs kernel
// (k_gfstack_runs) and k_gfstack_ws on float64 rows carry the epilogue; behind every other kernel -- and behind all of them
// under BEATAMD_QF_FUSE=0 (A/B, tests) -- the residuals are stored and k_quadform_band1 follows.
enum GfBand1 : int { GF_BY_NONE, GF_BY_COMBINE, GF_BY_RUNS, GF_BY_WS, GF_BY_QUADFORM };
inline GfBand1 gf_band1(bool carries, GfBand1 by, int *mode)   // mode 3 asked of a kernel -> who evaluates it, the kernel's mode
{
    if (!carries) *mode = GF_RESID_STORE;
    return carries ? by : GF_BY_QUADFORM;
}
enum GfStacker : int { GF_STREAMING, GF_RUNS, GF_GROUPS };
// one group size of the chain-shared (lane <-> chain) stackers: chains per group, distinct-row bound, epilogue mode, the
// kernel (k_gfstack_ws, loader / consumer, or the small-group k_gfstack_dma family)
struct GfGroup {
    int cg = 0, ucap = 0, mode = 0;
    bool ws = false;
    GfBand1 band1 = GF_BY_NONE;
};
struct GfPlan {
    const GfKnobs *knobs = nullptr;   // the knobs in force, read once per call
    // PATCH SPLIT (round 6, small-N libraries): the libraries are VIEWS [T*R, P/R, D, S, N] of the real ones (virtual
    // target t*R + r = target t, patches [r*P/R, (r+1)*P/R)), the tables are built per virtual slot and the stacking
    // kernels run unchanged on R times as many, R times shorter (target, tile) walks; slips / start times / durations
    // are read at the REAL patch r*P/R + p.
    int R = 1;
    int64_t T = 0, P = 0;             // the library as it is stacked: T*R targets of P/R patches
    bool tinv = false, slots = false; // index tables shared by all targets / by the targets of a station slot
    int64_t Ttab = 0;                 // table slots per chain
    int nrow = 1;                     // library rows per chain and patch (multilinear: 4)
    // float storage asked for and every library has its float copy; BEATAMD_GS_PAIR=1: k_gfstack_ws gathers ds_read_b128 pairs
    // (A/B); the kernels that have the bidiagonal epilogue use it (BEATAMD_QF_FUSE=0: none); 512-chain groups take k_gfstack_ws
    bool f32 = false, pair64 = false, fused = true, ws512 = false;
    GfStacker stacker = GF_STREAMING;
    // epilogue modes: of the runs kernel or the streaming kernel as the stacker, of the streaming kernel standing in for
    // the runs kernel (mode 3: followed by a guarded k_quadform_band1?), of k_split_combine (R > 1: the stackers get mode 0)
    int mode = 0, mode_standin = 0, mode_combine = 0;
    bool standin_band1 = false;
    GfBand1 band1 = GF_BY_NONE;       // who evaluates mode 3 (GF_GROUPS with R == 1: the GfGroup launched says)
    // GF_GROUPS: the group size in force, and the sizes to measure where it is measured (ctx->gs_tuned keeps the result)
    GfGroup group, cand[4];
    int ncand = 0;
    bool tune = false;
};
GfPlan gf_plan_call(const GfStackCall &call, const GfKnobs &kn, int num_cu);
// what a launch adds, products of the device and of the context's state: the table slot of a (virtual) target when targets
// share tables (device [T]), the index tables of k_gf_tables, GF_GROUPS: the group launched (the plan's or the measured one)
struct GfLaunch {
    const int32_t *tslot = nullptr;
    const uint32_t *rowoff = nullptr;
    const double *fac = nullptr;
    GfGroup group;
};
// what beatamd_ctx_gf_group_stats reports of a chain-shared launch
void gs_record_stats(beatamd_ctx *ctx, const GfStackCall &k, int64_t GTP, int64_t Ttab, int cg, bool has_passes);
// gfshared.hip: chain-shared variant (distinct rows staged once per chain group).  gfstack_shared_plan: false = no group
// size fits this call, else p.ws512, p.group, p.tune, p.cand; gfstack_group: the GfGroup of a size
bool gfstack_shared_plan(const GfStackCall &call, GfPlan &p);
GfGroup gfstack_group(const GfPlan &p, int cg, int ucap);
int launch_gfstack_shared(beatamd_ctx *ctx, const GfStackCall &call, const GfPlan &p, const GfLaunch &ln, const GfGroup &g);

// gfcell.hip: multilinear stacking with the rows of a cell in registers (518-chain groups, row passes): k_gfstack_runs.
// *ovf (device, nullable on return): nonzero after the launch = the tables overflowed and nothing was stacked -- the
// caller enqueues k_gfstack behind it as a stand-in guarded by the same flag
// the chains of a batch cut into ngroups groups of cg chain slots by recursive bisection along the key in which a part's
// chains spread wider (k_gc_cut): members[g * cg + i] = i-th chain of group g, ~0 behind the last chain (one workgroup
// sorting in LDS: C <= 8192, <= 64 groups); members = nullptr when the batch is larger or a key is missing
int launch_chain_members(beatamd_ctx *ctx, int64_t C, const ChainVec key[2], int64_t cg, int64_t ngroups, const uint32_t **members,
                         int strips = 0);
bool gfstack_ml_applicable(const GfStackCall &call, const GfPlan &p);
int launch_gfstack_ml(beatamd_ctx *ctx, const GfStackCall &call, const GfPlan &p, const GfLaunch &ln, const int **ovf);

// ---- quadform.hip ----------------------------------------------------------------
// quad[c,d] = || A_d x_{c,d} ||^2 ; A [nd or 1, M, M] row-major ; x(c,d,k) = X[c*xs_c + d*xs_d + k]
struct QuadformCall {
    const double *A = nullptr;
    int64_t a_stride = 0;  // elements between consecutive A_d (0: one shared A)
    int64_t M = 0, nd = 0, C = 0;
    const double *X = nullptr;
    int64_t xs_c = 0, xs_d = 0;
    int upper_tri = 0;
    double *quad = nullptr;  // [C, nd] with row stride q_stride
    int64_t q_stride = 0;
};
int launch_quadform(beatamd_ctx *ctx, const QuadformCall &call);
// banded upper-triangular operators (quadform.hip): the half bandwidth of a stack of matrices (entries beyond it are at most
// 2^-40 of their row's largest; scratch: nd * M * 8 + 16 bytes), the compact band [nd, M, band + 1], and the quadratic form on it
constexpr int QF_BAND_LIMIT = 16;
int launch_band_detect(beatamd_ctx *ctx, const double *A, int64_t nd, int64_t M, void *scratch, int64_t *band_host,
                       double *dropped_rel_host);
int launch_band_pack(beatamd_ctx *ctx, const double *A, int64_t nd, int64_t M, int64_t band, double *wb);
int launch_quadform_banded(beatamd_ctx *ctx, const double *wb, int64_t band, int64_t M, int64_t nd, int64_t C, const double *X,
                           int64_t xs_c, int64_t xs_d, double *quad, int64_t q_stride, const int *guard = nullptr, int want = 0);
// several small dense datasets (M <= 512 each) of one residual matrix in one launch, MVN epilogue
// included: LL[c*ld + d] = -0.5 (slog_d + M_d (2 h + log 2pi) + exp(-2h) |W_d x_{c,d}|^2), h = Q[c, hp_off_d]
struct QuadformSmallCall {
    int nd = 0;
    const double *A[8];
    int64_t M[8], xoff[8];
    int upper_tri[8];
    const double *slog[8];
    const int64_t *hp_off[8];
    int64_t C = 0;
    const double *X = nullptr;
    int64_t xs_c = 0;
    const double *Q = nullptr;
    int64_t nparams = 0;
    double *LL = nullptr;
    int64_t ld = 0;
    bool misfit_only = false;   // LL[c*ld + d] = |W_d x_{c,d}|^2 without the epilogue (slog, hp_off, Q unread)
};
bool quadform_small_applicable(int nd, const int64_t *M);
int launch_quadform_small(beatamd_ctx *ctx, const QuadformSmallCall &call);
int launch_check_upper_tri(beatamd_ctx *ctx, const double *A, int64_t nd, int64_t M, int *flag_dev);

// ---- logp.hip (small kernels: likelihood epilogues, geodetic stacking) -------------
struct HpSrc {  // hp(c,d) = base[c*stride + (offs ? offs[d] : d)]
    const double *base = nullptr;
    int64_t stride = 0;
    const int64_t *offs = nullptr;
};
// logpts[c*ld + d] = -0.5*(slog[d] + int16(M)*(2hp+log2pi) + (1/exp(2hp))*quad[c*nd+d]*wsq)
int launch_mvn_finish(beatamd_ctx *ctx, int64_t C, int64_t nd, int64_t M, const double *quad,
                      const double *slog, HpSrc hp, double *logpts, int64_t ld);
// scalar-weight quadratic form: quad[c,d] = sum_k (w_d * X[c,d,k])^2
int launch_scalar_quad(beatamd_ctx *ctx, int64_t C, int64_t nd, int64_t M, const double *X,
                       int64_t xs_c, int64_t xs_d, const double *w, double *quad);
// geodetic: mu[c,k] (+)= sum_p slips(c,p) G[p,k]
int launch_geo_stack(beatamd_ctx *ctx, const GeoLib *const *libs, int nvar, int64_t C, const ChainVec *slips, int accumulate,
                     double *mu);
// res[c,k] = (data[k] - mu[c,k]) * odw[k], minus the dataset's correction terms (gc.nterm > 0)
int launch_geo_residual(beatamd_ctx *ctx, int64_t C, int64_t Nobs, const double *data,
                        const double *odw, const double *mu, double *res, const double *Q = nullptr,
                        int64_t nparams = 0, GeoCorr gc = GeoCorr());

// corrections.hip: out [C, npole, 4] = the derived coefficients omega' p of every (chain, pole term) (k_pole_coef);
// euler_slips, coupling [C, P] of one pole against a patch basis Bp [P, 3] and the back-slip q[c, uparr_off + p]
int launch_pole_coef(beatamd_ctx *ctx, const PoleTerm *terms, int npole, const double *Q, int64_t nparams, int64_t C, double *out);
int launch_pole_coupling(beatamd_ctx *ctx, const PoleTerm &term, const double *Q, int64_t nparams, int64_t C, int64_t P,
                         const double *Bp, int64_t uparr_off, double *euler_slips, double *coupling);

// polarity.hip: one launch for all maps of the composite, a wavefront per chain.  out [C, ld]: the llk columns of the
// stations (POL_OUT_LLK), their amplitudes (POL_OUT_AMP) or the normalised m6 (POL_OUT_M6; rw, obs not read)
constexpr int POL_OUT_LLK = 0, POL_OUT_AMP = 1, POL_OUT_M6 = 2;
struct PolArgs {
    PolSource src;
    int32_t nmap = 0, mode = POL_OUT_LLK, ntab = 0, pad_ = 0;
    int64_t NT = 0;
    int64_t map_end[POL_MAX_MAPS] = {};
    int64_t hp_off[POL_MAX_MAPS] = {};
    double hp_fix[POL_MAX_MAPS] = {};
    double gamma = 0.2;
    const double *rw = nullptr, *obs = nullptr, *utab = nullptr, *btab = nullptr;
    const double *Q = nullptr;
    int64_t nparams = 0, C = 0;
    const int32_t *active = nullptr;   // device [C] or nullptr: chains with 0 are skipped
    double *out = nullptr;
    int64_t ld = 0;
};
int launch_polarity(beatamd_ctx *ctx, const PolArgs &a);
// out[i] = w_to_beta(w[i]) on the tables (sources.py:379-392), the device function of k_polarity
int launch_w_to_beta(beatamd_ctx *ctx, int64_t n, const double *w, const double *utab, const double *btab, int ntab, double *out);

#ifdef __HIPCC__
// The weighted residual of observation k of chain c with the correction terms of k's dataset subtracted one after the
// other in table order (geodetic.py:1072-1077, 411-427):
//     corr = ((B[k,0]*coef0 + B[k,1]*coef1) + B[k,2]*coef2) + B[k,3]*coef3 ;  res = ((d - mu) * odw) - corr
// with plain products and sums (no contraction, whatever the including file's default): for a ramp, whose last column
// is 1, that is numpy's (d - mu)*odw - (locy*az + locx*rg + off) bit for bit.
// The term table is the same for every lane: it is read through the constant address space, i.e. scalar loads.  The
// coefficients q[c, off] are wave-uniform wherever the wavefront lies inside one chain (the flat (chain, observation)
// index lets a wavefront straddle two): that wavefront reads them through scalar loads from the first lane's chain,
// a straddling one per lane.  The basis columns are the only per-lane loads either way.
// A pole term (kind 1) takes its three coefficients from the chain's derived records Pc = gc.pole + c * gc.pole_stride
// (k_pole_coef wrote them ahead of this kernel) instead of q, through the same kind of load; the products, the sum
// order and the subtraction are the same lines.
template <bool UNIFORM>
__device__ __forceinline__ double geo_corr_subtract(const GeoCorr &gc, const double *Qc, const double *Pc, int64_t k, double r)
{
#pragma clang fp contract(off)
    typedef const __attribute__((address_space(4))) GeoCorrTerm *TermPtr;
    typedef const __attribute__((address_space(4))) double *ConstPtr;
    TermPtr terms = (TermPtr)gc.terms;
    for (int j = 0; j < gc.nterm; j++) {
        // the whole row and all four coefficient slots at once, ahead of any branch: the compiler batches them into
        // three rounds of scalar loads per term instead of one per field (an unused slot has offset -1 and the fixed
        // value 0; q[0] stands in for its load)
        struct { int64_t start, n; const double *B; int64_t off[4]; double fix[4]; int K, kind, rec; } t;
        t.start = terms[j].start; t.n = terms[j].n; t.B = terms[j].B; t.K = terms[j].K;
        t.kind = terms[j].kind; t.rec = terms[j].rec;
#pragma unroll
        for (int kk = 0; kk < 4; kk++) { t.off[kk] = terms[j].off[kk]; t.fix[kk] = terms[j].fix[kk]; }
        double coef[4];
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            const int64_t o = t.off[kk] < 0 ? 0 : t.off[kk];
            const double q = UNIFORM ? ((ConstPtr)Qc)[o] : Qc[o];
            coef[kk] = t.off[kk] < 0 ? t.fix[kk] : q;
        }
        if (t.kind == GEO_CORR_POLE) {   // (the same for every lane)
            const double *P = Pc + (int64_t)t.rec * 4;
#pragma unroll
            for (int kk = 0; kk < 4; kk++) coef[kk] = UNIFORM ? ((ConstPtr)P)[kk] : P[kk];
        }
        const int64_t row = k - t.start;
        if (row < 0 || row >= t.n) continue;
        // columns beyond K: column 0 is read in their place and the sum is not taken
        const double *B = t.B + row;
        const double p0 = B[0] * coef[0];
        const double p1 = B[(t.K > 1 ? 1 : 0) * t.n] * coef[1];
        const double p2 = B[(t.K > 2 ? 2 : 0) * t.n] * coef[2];
        const double p3 = B[(t.K > 3 ? 3 : 0) * t.n] * coef[3];
        double corr = p0;
        corr = t.K > 1 ? corr + p1 : corr;
        corr = t.K > 2 ? corr + p2 : corr;
        corr = t.K > 3 ? corr + p3 : corr;
        r = r - corr;
    }
    return r;
}

__device__ __forceinline__ double geo_corrected_residual(const GeoCorr &gc, const double *Q, int64_t nparams, int64_t c,
                                                         int64_t k, double d, double mu, double odw)
{
#pragma clang fp contract(off)
    const double r = (d - mu) * odw;
    const int c0 = __builtin_amdgcn_readfirstlane((int)c);
    if (__all(c == (int64_t)c0))
        return geo_corr_subtract<true>(gc, Q + (int64_t)c0 * nparams, gc.pole + (int64_t)c0 * gc.pole_stride, k, r);
    return geo_corr_subtract<false>(gc, Q + c * nparams, gc.pole + c * gc.pole_stride, k, r);
}
#endif
// the hyper model's cached misfits: dst[c*ld + k] = src[c*n + k], k < n; then NaN into the rows of flagged chains
int launch_store_misfits(beatamd_ctx *ctx, int64_t C, int64_t n, const double *src, double *dst, int64_t ld);
int launch_misfits_mark_bad(beatamd_ctx *ctx, int64_t C, int64_t n, double *llks, const int32_t *chain_bad);
// laplacian: out[c*ld] = sum_v -0.5*(-logdet + P*(log2pi+2h) + (1/exp(2h))*quad[c,v])
int launch_laplacian_finish(beatamd_ctx *ctx, int64_t C, int64_t nvar, int64_t P, double logdet,
                            const double *quad, HpSrc hp, double *out, int64_t ld);
// LL[c, nllk-1] = sum of composite sums (problems.py:227-247)
struct LikeGroups {  // composite boundaries inside the llk vector (exclusive ends)
    int32_t end[8];
    int n = 0;
};
// chain_bad (nullable): chains flagged by the index maps / the sweep get like = NaN
int launch_like_sum(beatamd_ctx *ctx, int64_t C, int64_t nllk, const LikeGroups &grp, double *LL,
                    const int32_t *chain_bad);
// likelihood vectors of a target-sharded model from the all-gathered rows of the ranks (k_like_assemble, logp.hip)
int launch_like_assemble(beatamd_ctx *ctx, int64_t C, int64_t nllk, int64_t nsrc, const double *src, const int32_t *dst_col,
                         const double *rest, int64_t rest_ld, int64_t rest_col0, int64_t n_rest, int64_t rest_dst0,
                         const LikeGroups &grp, double *LL, int32_t *chain_bad);
// gather slips of all variables into a dense [C, nvar, P] buffer
int launch_gather_slips(beatamd_ctx *ctx, int64_t C, int nvar, int64_t P, const ChainVec *slips,
                        double *out);
// geometry.hip: line-of-sight synthetics of rectangular / Mogi sources, mu [C, Nobs]
// with res (and data, odw [Nobs]): res = (data - mu) * odw is stored instead of mu, minus the correction terms gc
int launch_geom_los(beatamd_ctx *ctx, const GeomSources &g, const double *Q, int64_t nparams,
                    int64_t C, double *mu, const double *data = nullptr, const double *odw = nullptr,
                    double *res = nullptr, GeoCorr gc = GeoCorr());
// displacement components (n, e, up) per (parameter set, source, point): out [C, nsrc, Nobs, 3]
int launch_geom_disp(beatamd_ctx *ctx, int nsrc, const int32_t *kind, const int64_t *poff,
                     const double *params, int64_t C, int64_t nobs, const double *east,
                     const double *north, double nu, double *out);
// geolib.hip: G [nrows, nobs] = line-of-sight displacement * odw of nrows unit sources (params [nrows, 10]; kind / poff
// describe one rectangular source with identity offsets); everything on the device
int launch_geo_gf_library(beatamd_ctx *ctx, int64_t nrows, const double *params, const int32_t *kind,
                          const int64_t *poff, int64_t nobs, const double *east, const double *north,
                          const double *los, const double *odw, double nu, double *G);
// resolution.hip (device pointers): the correlated smoothing operator (kind 0 gaussian, 1 exponential), the model
// resolution matrix R [P, P] with its diagonal, and the division rating (dmin [P]: scratch and by-product)
int launch_smoothing_correlated(beatamd_ctx *ctx, int64_t P, const double *coords, int kind, double *L);
int launch_model_resolution(beatamd_ctx *ctx, int64_t P, int64_t nobs, const double *gfs, const double *L,
                            double epsilon, double *R, double *diag);
int launch_division_rating(beatamd_ctx *ctx, int64_t P, int64_t nobs, const double *widths, const double *lengths,
                           const double *centers, const double *bottom_depth, double depth_penalty,
                           const double *data_en, const double *mean_R, double *dmin, double *rating);
// covariance.py:716-771 on device
int launch_autocovariance(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *data,
                          const double *mean, double *out);
int launch_scaled_toeplitz(beatamd_ctx *ctx, int64_t nd, int64_t n, const double *coeffs,
                           const double *stds, double *out);


// ---- gemm.hip: O[m,n] = (sum_k A[m,k] Bop[k,n]) * row_scale[m] on the FP64 matrix cores
struct GemmCall {
    const double *A = nullptr, *B = nullptr, *row_scale = nullptr;
    double *O = nullptr;
    int64_t lda = 0, ldb = 0, ldo = 0, M = 0, N = 0, K = 0;
    int b_kn = 0;     // 0: Bop[k,n] = B[n*ldb + k] ("NT")   1: Bop[k,n] = B[k*ldb + n] ("NN")
    int b_upper = 0;  // NT only: B[n,k] == 0 for k < n
    const char *timer = nullptr;
    // batched / accumulating form (chol.hip): O = alpha * A.Bop (+ O); matrices sA/sB/sO apart
    int nbatch = 1;
    int64_t sA = 0, sB = 0, sO = 0;
    int64_t sR = 0;   // row_scale entries between the matrices of a batch
    double alpha = 1.0;
    int accumulate = 0;
    int lower_only = 0;   // M == N: tiles strictly above the diagonal are skipped
    int b_lower = 0;      // NN only: Bop[k,n] == 0 for k < n
    int col_block = -1;   // >= 0: only this 128-column block of the product (in-place whitening)
};
int launch_gemm_f64(beatamd_ctx *ctx, const GemmCall &call);
// chol.hip: W = cholesky(inv(C)).T and log det C of a stack of matrices (device pointers)
// notpsd (nullable, device [nbatch]): per-matrix flag instead of the status word for a matrix that is not
// positive definite (its W / log_pdet are then meaningless)
int launch_chol_inverse(beatamd_ctx *ctx, int64_t nbatch, int64_t n, const double *C, double *W, double *log_pdet,
                        int32_t *notpsd = nullptr);
// R [n,n] upper triangular with R^T R = F^T F for a tall F [K,n] (device pointers)
int launch_gram_cholesky(beatamd_ctx *ctx, int64_t K, int64_t n, const double *F, double *R);
// M = Wn . inv(Wo) for stacks of upper-triangular matrices (device pointers)
int launch_triu_ratio(beatamd_ctx *ctx, int64_t nbatch, int64_t n, const double *Wn, const double *Wo, double *M);
// lower Cholesky factors of the padded matrices A [nbatch][np][np] in place (np a multiple of 64, identity in the
// padding; lower triangles read); notpsd [nbatch] (device) = 1 where a pivot was not positive
int launch_potrf_lower(beatamd_ctx *ctx, int64_t nbatch, int64_t np, double *A, int32_t *notpsd);
// X[b, :] = inv(W[b]) . X[b, :] for upper-triangular W (one vector per matrix, back substitution)
int launch_triu_solve_vec(beatamd_ctx *ctx, int64_t nbatch, int64_t n, const double *W, double *X);

// ---- smc.hip: sampler steps on the device (stage transition, draws, propose / accept, tuning)
int launch_smc_calc_beta(beatamd_ctx *ctx, int64_t n, const double *lik, int64_t stride, double beta,
                         double cv, int mode, double dbeta, double *out2, double *weights);
int launch_smc_resample(beatamd_ctx *ctx, int64_t n, const double *weights, double aux, double *cum,
                        int32_t *idx);
int launch_pop_factor(beatamd_ctx *ctx, int64_t n, int64_t np, const double *X, int64_t ldx,
                      const double *w, double *F);
int launch_gather_rows(beatamd_ctx *ctx, int64_t nout, int64_t ncol, const double *src, int64_t lds,
                       int64_t nrow_src, const int32_t *idx, double *out, int64_t ldo);
int launch_tune_scaling(beatamd_ctx *ctx, int64_t C, double *scaling, int32_t *accepted, double interval);
int launch_accumulate_i32(beatamd_ctx *ctx, int64_t C, const int32_t *a, int32_t *acc);
int launch_philox_normal(beatamd_ctx *ctx, double *z, int64_t C, int64_t K, uint64_t seed,
                         uint32_t step, uint64_t first_chain);
int launch_philox_univariate(beatamd_ctx *ctx, double *delta, int64_t C, int64_t np, int kind,
                             const double *scale, uint64_t seed, uint32_t step, uint64_t first_chain);
int launch_step_advance(beatamd_ctx *ctx);
// small parameter vectors (K, np <= 64): draws + factor product + propose in one launch; kind -1
// multivariate (factor [K, np]), 0..3 the per-parameter families (factor = scales [np], K == np)
// groups > 1 (multivariate; C a multiple of it): factor [groups, K, np], chain c draws with factor c / (C / groups)
bool draw_propose_applicable(int64_t K, int64_t np);
int launch_draw_propose(beatamd_ctx *ctx, int64_t C, int64_t K, int64_t np, int kind, const double *factor,
                        int df, uint64_t seed, uint32_t step, uint64_t first_chain, const double *Q0,
                        const double *scaling, const double *lower, const double *upper, double *Qprop,
                        double *log_u, int32_t *inbounds, int64_t groups = 1);
int launch_philox_chain(beatamd_ctx *ctx, int64_t C, uint64_t seed, uint32_t step, uint64_t first_chain,
                        int df, double *log_u, double *row_scale);
// the step around the forward model (metropolis.py:276-422 pieces): propose before it, accept behind it
int launch_propose(beatamd_ctx *ctx, int64_t C, int64_t nparams, const double *Q0,
                   const double *delta, const double *scaling, const double *lower,
                   const double *upper, double *Qprop, int32_t *inbounds);
// grp (nullable): sum the `like` column of Lprop here instead of a launch_like_sum before; acc_sum /
// n_acc (nullable): per-chain and population acceptance counters; advance_step: bump ctx->step_dev
int launch_accept(beatamd_ctx *ctx, int64_t C, int64_t nparams, int64_t nllk, double *Q0,
                  double *L0, const double *Qprop, double *Lprop, const int32_t *inbounds,
                  const double *log_u, double beta, const double *betas, int32_t *accepted,
                  const LikeGroups *grp = nullptr, const int32_t *chain_bad = nullptr,
                  int32_t *acc_sum = nullptr, int64_t *n_acc = nullptr, bool advance_step = false);


// ---- hyper.hip: the hyper-parameter model on cached misfits
// LL[c, :] = (terms, like) of H [C, nh] given llks [C, nterm]   (k_hyper_logp)
int launch_hyper_logp(beatamd_ctx *ctx, const HyperModel &m, int64_t C, const double *H, const double *llks, double *LL);
// n_steps Metropolis steps of every chain in one launch (k_hyper_chain); device pointers
constexpr int HYPER_CHAIN_MAX = 1024;   // hyper-parameters and terms a chain's wavefront holds in LDS, each
struct HyperChainCall {
    int64_t C = 0, n_steps = 0;
    double *H = nullptr, *LL = nullptr, *scaling = nullptr;
    int32_t *acc_since = nullptr;
    const double *llks = nullptr, *lower = nullptr, *upper = nullptr, *scales = nullptr;
    int kind = 0;
    uint64_t seed = 0, first_chain = 0;
    uint32_t step0 = 0;
    int tune_interval = 0, steps_until_tune = 0, buffer_thinning = 1;
    double *trace = nullptr;
    int64_t *n_acc = nullptr;
};
bool hyper_chain_applicable(int64_t nh, int64_t nterm);
int launch_hyper_chain(beatamd_ctx *ctx, const HyperModel &m, const HyperChainCall &call);

// ---- summary.hip: posterior diagnostics of a population
// VR[c*n + k] = 1 - nom[c*ld + k] / denom[k]   (k_variance_reduction)
int launch_variance_reduction(beatamd_ctx *ctx, int64_t C, int64_t n, const double *nom, int64_t ld, const double *denom,
                              double *VR);
// out[c,t,k] = exp(-hp[c,t]) * (S[t] * X[c,t,k]); S / hp nullable (k_standardize); X may be out
int launch_standardize(beatamd_ctx *ctx, int64_t C, int64_t T, int64_t N, const double *S, const double *hp, const double *X,
                       double *out);
// Welford update of state [5, M] = (mean, M2, min, max, spare) with the rows of X [C, M] in row order, n_seen rows before
// them (k_ensemble_moments); mean / sqrt(M2 / n) / min / max out of the state (k_moments_finish)
int launch_ensemble_moments(beatamd_ctx *ctx, int64_t C, int64_t M, const double *X, double *state, int64_t n_seen);
int launch_moments_finish(beatamd_ctx *ctx, int64_t M, const double *state, int64_t n, double *mean, double *std, double *mn,
                          double *mx);
// grid [T,ny,nx] += the line images of the traces Y [E,T,N] in ensemble order (k_trace_density_check, k_trace_density);
// an index outside the grid or a non-finite sample raises the status word
int launch_trace_density(beatamd_ctx *ctx, int64_t E, int64_t T, int64_t N, const double *Y, const double *tmin, double deltat,
                         const double *extent, int64_t ny, int64_t nx, double linewidth, double *grid);

// the same with per-trace sample ranges [E,T,2] = (first sample, count) (nullptr: every sample): only the segments inside
// a trace's own range are drawn, a trace with count < 2 draws nothing
int launch_trace_density(beatamd_ctx *ctx, int64_t E, int64_t T, int64_t N, const double *Y, const double *tmin, double deltat,
                         const double *extent, int64_t ny, int64_t nx, double linewidth, double *grid, const int64_t *ranges);

// ---- momentrate.hip: moment, magnitude and moment-rate function of every draw (ffi/fault.py:284-474)
// the slip components a moment is formed from: offsets in q of n variables of P entries each
struct MrComps {
    int64_t off[4];
    int32_t n;
};
constexpr int MR_NT_MAX = 20224;   // samples of a moment-rate row: 158 KiB of the 160 KiB of LDS
// M0 [C] = sum_p k_p sqrt(sum_comp s^2) in patch order, Mw [C] (k_moment_magnitude)
int launch_moment_magnitude(beatamd_ctx *ctx, int64_t C, int64_t P, const double *Q, int64_t np, const MrComps &comps,
                            const double *k, double *M0, double *Mw);
// spans [C, nsub + 1, 2] = (first index, count) of every subfault's and the total's time axis (k_moment_rate_span)
int launch_moment_rate_span(beatamd_ctx *ctx, const FfiModel &m, int64_t C, const double *Q, const double *st0,
                            const int32_t *chain_bad, double deltat, int64_t *spans);
// out [C, nsub + 1, NT] on the index grid [kbase, kbase + NT): the subfaults' rows (k_moment_rate) and their in-order sum
// (k_moment_rate_total)
int launch_moment_rate(beatamd_ctx *ctx, const FfiModel &m, int64_t C, const double *Q, const double *st0, const MrComps &comps,
                       const double *k, double deltat, const int64_t *spans, int64_t kbase, int64_t NT, double *out);

// ---- ptadapt.hip: streaming likelihood-weighted moments of groups of chains and the proposal factors out of them
// state of a group: GM_HDR header doubles (m, S0, Sw2, count, nbad, 3 spare), S1 [n], S2 [n, n] (lower triangle)
constexpr int GM_HDR = 8, GM_MAX_R = 1024, GM_MAX_N = 2048, GM_MAX_G = 64;
inline int64_t group_moments_stride(int64_t n) { return GM_HDR + n + n * n; }
// empty state; ref (nullable) [G, n] = mean of the R rows of every group of Q
int launch_group_moments_reset(beatamd_ctx *ctx, int64_t G, int64_t n, double *state, int64_t R, const double *Q, double *ref);
// the R rows of every group (rows g R .. g R + R - 1 of Q [G R, n]; like[(g R + r) like_stride]; ref [G, n]) into state
int launch_group_moments_update(beatamd_ctx *ctx, int64_t G, int64_t R, int64_t n, const double *Q, const double *like,
                                int64_t like_stride, const double *ref, double *state);
// factor [G, n, n] upper with F^T F = cov, cov [G, n, n] (nullable), flags [G]: 0 ok, 1 bad moments, 2 not positive definite
// (the factor of a flagged group is not written)
int launch_group_moments_factor(beatamd_ctx *ctx, int64_t G, int64_t n, const double *state, double *factor, double *cov,
                                int32_t *flags);

// ---- predcov.hip: velocity-model prediction covariance of the geodetic datasets (geodetic.py:1130-1202)
// X[k, :] = sum_v G_{k,v}.T . slips_v for the K variants of a library ensemble (k_crust_stack); G: device table [K * nvar],
// variant-major; slips [nvar * P]
int launch_crust_stack(beatamd_ctx *ctx, const double *const *G, int64_t K, int nvar, int64_t P, int64_t Nobs,
                       const double *slips, double *X);
// out_i = base_i + cov(X[:, o_i : o_i + n_i], rowvar=0) for the datasets of a composite in one launch (k_pred_center,
// k_pred_cov); D [K, Nobs]: device scratch for the centred columns; sets: device table [nd], nmax = the largest n_i
struct PredCovSet {
    int64_t off, n;        // first column of the dataset in X, its size
    const double *base;    // device [n, n] or nullptr (zeros)
    double *out;           // device [n, n]
};
int launch_pred_covariance(beatamd_ctx *ctx, int64_t K, int64_t Nobs, const double *X, double *D, int64_t nd, int64_t nmax,
                           const PredCovSet *sets);

// ---- noise2d.hip: the 2-d neighbourhood statistic of the geodetic "non-toeplitz" noise structure (covariance.py:774-811)
// radius [nd], counts / stds [Ntot] of the datasets of a composite in one call (k_ball_maxd2, k_ball_radius, k_ball_rms);
// sets: device table [nd], nmax = the largest n; pmax [Ntot]: device scratch for the per-point largest squared distance
struct BallSet {
    int64_t off, n;   // first point of the dataset in the concatenated arrays, its size
};
int launch_ball_rms(beatamd_ctx *ctx, int64_t nd, int64_t nmax, const BallSet *sets, const double *coords, const double *data,
                    double max_dist_perc, double *pmax, double *radius, int32_t *counts, double *stds);

// ---- spectrum.hip: amplitude spectra abs(rfft(x, ntrans))[lo:hi] of rows of real samples (heart.py:4091-4155)
constexpr int SPEC_NTRANS_MIN = 2, SPEC_NTRANS_MAX = 8192;
constexpr int SPEC_WAVE_NTRANS = 512;   // up to here one wavefront per trace, four traces per workgroup; above one workgroup
// 0 <= lo < hi <= ntrans/2 + 1, 1 <= N <= ntrans, ntrans a power of two in [SPEC_NTRANS_MIN, SPEC_NTRANS_MAX]
int spectrum_check_band(int64_t N, int64_t ntrans, int64_t lo, int64_t hi);
// *W = the context's table exp(-2 pi i k / ntrans), k < ntrans/2, made on first use (never inside a graph capture)
int spectrum_twiddles(beatamd_ctx *ctx, int64_t ntrans, const double **W);
// out [R, hi - lo] = spec(x_r) of the rows X[r*xs .. r*xs + N), or data_spec[r mod T] - spec(x_r) (data_spec [T, hi - lo])
int launch_amp_spectrum(beatamd_ctx *ctx, int64_t R, int64_t N, int64_t xs, int64_t ntrans, int64_t lo, int64_t hi,
                        const double *X, const double *data_spec, int64_t T, double *out);

// ---- lsq.hip: non-negative least-squares slip of a batch of chains (problems.py:753-873)
// the index tables of a stacking call, one per target (k_gf_tables): rowoff [C,T,P,nrow], fac [C,T,P,4] (multilinear)
int launch_gf_tables(beatamd_ctx *ctx, const GfStackCall &call, uint32_t *rowoff, double *fac);
// N [C,P,P] (the 64 x 64 tiles of the lower triangle) and b [C,P] (+)= sum_t R_t R_t^T, sum_t R_t d_t of one library
// (k_lsq_gram, k_lsq_rhs); accumulate: continue the stored sums
int launch_lsq_seismic(beatamd_ctx *ctx, const SeisLib &lib, int interp, int64_t C, const uint32_t *rowoff, const double *fac,
                       const double *data, int accumulate, double *Nmat, double *b);
int launch_lsq_transpose(beatamd_ctx *ctx, const double *A, double *At, int64_t n);
// N += GG + h^4 LtL on the lower triangle, mirrored; b += Ggeo (dgeo - corr_c) (k_lsq_finish); GG / Ggeo nullable
int launch_lsq_finish(beatamd_ctx *ctx, int64_t C, int64_t P, double *Nmat, double *b, int has_seis, const double *GG,
                      const double *LtL, const double *Ggeo, int64_t Nobs, const double *dgeo, GeoCorr corr, const double *Q,
                      int64_t nparams, int64_t h_off);
// Lawson-Hanson active set per chain (k_nnls); maxiter <= 0: 3 n.  The factors of one launch stay within
// NNLS_SCRATCH_BYTES: larger batches run in chunks of chains
constexpr int NNLS_MAX_N = 1024;
constexpr int64_t NNLS_SCRATCH_BYTES = (int64_t)256 << 20;
int launch_nnls(beatamd_ctx *ctx, int64_t C, int64_t n, const double *Nmat, const double *b, double *x, int32_t *iters,
                int32_t *status, int maxiter);
int launch_lsq_scatter(beatamd_ctx *ctx, int64_t C, int64_t P, const double *x, double *Qout, int64_t nparams, int64_t v_off,
                       int64_t zero_off);

// ---- marginals.hip: sorted columns, percentiles, 1-d and 2-d counts and pairwise KDEs of a population X [n, V]
// (plotting/common.py:248-461, plotting/marginals.py:131-609)
constexpr int MG_SORT_TILE = 16384;                    // doubles of a column sorted in LDS by one workgroup (128 KiB)
constexpr int64_t MG_SORT_MAX_N = (int64_t)1 << 24;    // longest column
constexpr int MG_HIST2D_MAX_CELLS = 128 * 128, MG_HIST2D_MAX_SIDE = 4096;   // the LDS grid of k_pair_hist2d
constexpr int MG_NMOM = 9;                             // doubles per pair of k_pair_moments
constexpr int MG_KDE_SB = 1024;                        // samples of a block staged in LDS
constexpr int MG_KDE_G = 4, MG_KDE_TILE = MG_KDE_G * 256;   // grid points per lane and per workgroup
constexpr double MG_KDE_SKIP = 745.2;                  // exp(-x) is an exact zero above
inline int64_t kde_sample_blocks(int64_t n) { return (n + MG_KDE_SB - 1) / MG_KDE_SB; }
struct KdePair {
    double mx, my;          // the column means
    double l11, l21, l22;   // lower Cholesky factor of cov * n^(-1/3)
    double scale;           // 1 / (2 pi n l11 l22)
    int32_t ok, pad;        // 0: no factor, Z of the pair is NaN
};
// flags [K] = 1 where column cols[k] holds a non-finite sample
int launch_col_check(beatamd_ctx *ctx, const double *X, int64_t n, int64_t V, const int64_t *cols, int64_t K, int32_t *flags);
// out [K, n] = the columns cols[k] ascending
int launch_col_sort(beatamd_ctx *ctx, const double *X, int64_t n, int64_t V, const int64_t *cols, int64_t K, double *out);
// out [K, Q] = numpy.percentile(., q) of the sorted columns S [K, n]
int launch_col_percentiles(beatamd_ctx *ctx, const double *S, int64_t K, int64_t n, const double *q, int64_t Q, double *out);
// counts [K, nb] of the sorted columns on the edges [K, nb + 1] (non-decreasing rows)
int launch_col_hist(beatamd_ctx *ctx, const double *S, int64_t K, int64_t n, const double *edges, int64_t nb, int64_t *counts);
// counts [P, bx, by] of the pairs [P, 2] on xedges [P, bx + 1], yedges [P, by + 1]
int launch_pair_hist2d(beatamd_ctx *ctx, const double *X, int64_t n, int64_t V, const int64_t *pairs, int64_t P, int bx, int by,
                       const double *xedges, const double *yedges, int64_t *counts);
// mom [P, MG_NMOM]: means, centred second sums, extents
int launch_pair_moments(beatamd_ctx *ctx, const double *X, int64_t n, int64_t V, const int64_t *pairs, int64_t P, double *mom);
// Z [P, gx, gy]; W [P, n, 2], box [P, kde_sample_blocks(n), 4]: device scratch; grid [P, gx + gy]; skip: 0 adds every block;
// shape: 0 chosen by the launcher, 1 wide (MG_KDE_G points per lane, 256 lanes), 2 narrow (one point per lane, 64 lanes)
int launch_pair_kde2d(beatamd_ctx *ctx, const double *X, int64_t n, int64_t V, const int64_t *pairs, int64_t P,
                      const KdePair *par, double *W, double *box, const double *grid, int gx, int gy, int skip, int shape,
                      double *Z);
// U [n, 3]: unit vectors of (lat, lon) in degrees; transform: vonmises_fisher's 90 - lat and mod 360 (0: vonmises_std's none)
int launch_sph_unit(beatamd_ctx *ctx, int64_t n, const double *lat, const double *lon, int transform, double *U);
// S [3] = sum of the rows of U [n, 3] in a fixed order
int launch_sph_sum(beatamd_ctx *ctx, int64_t n, const double *U, double *S);
// kde [m] = sum_i exp(norm + Ug . U0_i / sigma2)
int launch_sph_kde(beatamd_ctx *ctx, int64_t n, const double *U0, int64_t m, const double *Ug, double norm, double sigma2,
                   int shape, double *kde);

// ---- convergence.hip: ESS, R-hat and highest-density intervals of a trace X [C, D, V] (apps/beat.py:1338-1363,
// backend.py:1401-1415)
constexpr int CV_NT = 6;                    // row sets of a variable: raw, squared deviation, <= q05, <= q95, z raw, z folded
constexpr int CV_NCOL = 11;                 // columns of the summary table
constexpr int CV_ACOV_TILE = 512;           // values of a row staged in LDS at a time by k_acov_lags
constexpr int64_t CV_ACOV_CHUNK = 4096;     // consecutive i summed into one partial sum of a lag: part of what a lag's bits are
constexpr int64_t CV_WORKSPACE_BYTES = (int64_t)1 << 30;   // the budget that sizes a batch of variables
constexpr int64_t CV_PART_BYTES = (int64_t)256 << 20;      // the chunk sums of one range of lags (k_acov_lags -> k_acov_combine)
// out [R, nlags] = the biased autocovariance of the rows Y [R, n] at the lags lag0 .. lag0 + nlags
int launch_autocov_lags(beatamd_ctx *ctx, int64_t R, int64_t n, const double *Y, int64_t lag0, int64_t nlags, double *out);
// z [n] (and ranks [n] unless NULL) of A [n]
int launch_rank_normalize(beatamd_ctx *ctx, int64_t n, const double *A, double *z, double *ranks);
// the variables of a pass when the caller fixes none
int64_t convergence_batch(int64_t C, int64_t D, int64_t K);
// out [K, CV_NCOL], flags [K], cols [K]: device; rounds: host, nullable
int launch_convergence_summary(beatamd_ctx *ctx, int64_t C, int64_t D, int64_t V, const double *X, int64_t K,
                               const int64_t *d_cols, double hdi_prob, double tau_floor, int64_t var_batch, int64_t first_lags,
                               double *out, int32_t *flags, int64_t *rounds);

// ---- mechanisms.hip: eigen-systems, standard decompositions, Hudson points and fuzzy-beachball grids of an ensemble of
// moment tensors (plotting/seismic.py:1334-1425, 1664-1850, 2183-2310); the per-draw arithmetic is mechanism.hpp's
constexpr int MC_NPART = 5;                                  // iso, dc, clvd, dev, full
constexpr int MC_G = 4, MC_TILE = MC_G * 256;                // pixels per lane and per workgroup of the wide shape
constexpr int64_t MC_CHUNK = 512;                            // draws a workgroup of k_fuzzy_accum counts before its atomics
constexpr int64_t MC_MAX_N = (int64_t)1 << 24;               // draws of a call
constexpr int MC_MAX_RES = 4096;                             // pixels a side of the focal-sphere grid
// *bad (device) = the first row of X [n, 6] (kind 0) / [n, 3] (kind 1) that is non-finite or, kind 0, all zero; 0xffffffff
int launch_mt_check(beatamd_ctx *ctx, const double *X, int64_t n, int kind, uint32_t *bad);
// evals [n, 3], evecs [n, 3, 3], moments, ratios [n, 5], parts, unit [n, 5, 6], uv [n, 2]; each may be NULL
int launch_mt_decompose(beatamd_ctx *ctx, int64_t n, int kind, const double *X, double *evals, double *evecs, double *moments,
                        double *ratios, double *parts, double *unit, double *uv);
// amps [P, cells] = NaN, then count / n (mask) or sum / n at pixel_index [npix]; unit [n, P, 6], rw [6, npix]; count
// [P, npix] (mask) and sum [P, npix] (!mask): device scratch; shape: 0 chosen here, 1 wide, 2 narrow
int launch_fuzzy_amps(beatamd_ctx *ctx, int64_t n, int P, const double *unit, int64_t npix, const double *rw,
                      const int64_t *pixel_index, int64_t cells, int mask, int shape, uint32_t *count, double *sum, double *amps);

// ---- rupture.hip: contour lines of the start times of an ensemble and the density grid of polylines (plotting/ffi.py:338-398,
// :599-615; plotting/common.py:619-801)
constexpr int CT_LMAX = 16;                 // levels of a (draw, subfault): matplotlib's automatic rule gives at most 10
constexpr int CT_SUB_FIELDS = 5;            // int64 per subfault: n_dip, n_strike, first patch, first x, first y
constexpr int CT_MAX_NODES = 2304;          // patches of a subfault (48 x 48): 56 bytes of LDS each, see ct_lds_bytes
// LDS of a wavefront of the contour kernels: the start times (8 bytes a node) and six int tables of two slots a cell
inline size_t ct_lds_bytes(int64_t nodes) { return (size_t)nodes * (8 + 2 * 6 * 4); }
constexpr int PD_STRIP = 32, PD_ROWS = 64;  // the tile of a workgroup of k_polyline_density: columns x rows
constexpr int PD_LDS_BYTES = 150 * 1024;    // the owner map's share of LDS
// out [E, nsub, 2] = (min, max) of every (draw, subfault), both NaN where a start time is not finite (k_rupture_minmax)
int launch_rupture_minmax(beatamd_ctx *ctx, int64_t E, int64_t ncells_total, const double *sts, int nsub, const int64_t *subs,
                          double *out);
// counts != nullptr: the count pass, counts [E, nsub, CT_LMAX, 2] = (lines, vertices) (k_contour_count); else the fill pass
// with the exclusive scans line_base / vert_base [E, nsub, CT_LMAX] (k_contour_fill).  max_nodes: the largest subfault
int launch_contours(beatamd_ctx *ctx, int64_t E, int64_t ncells_total, const double *sts, int nsub, const int64_t *subs,
                    int64_t max_nodes, const double *x, const double *y, const double *levels, const int32_t *nlevels,
                    int32_t *counts, const int64_t *line_base, const int64_t *vert_base, int64_t nlines, int64_t nverts, double *vertices,
                    int64_t *line_offsets);
// grid [ny, nx] += the images of the polylines sel [nsel] (nullptr: 0 ... nsel - 1) in that order, coverage (nullable) += 1
// per polyline where its image is positive (k_polyline_check, k_polyline_density); extent: host (xmin, xmax, ymin, ymax)
int launch_polyline_density(beatamd_ctx *ctx, int64_t nsel, const int64_t *sel, const int64_t *line_offsets,
                            const double *vertices, const double *extent, int64_t ny, int64_t nx, double linewidth, double *grid,
                            int32_t *coverage);

// ---- seislib.hip: the producer of the seismic FFI library (ffi/base.py:1005-1254, heart.py:3466-3525, 4242-4323); the
// arithmetic contract stands at the head of seislib.hip
constexpr int SL_MAX_STAGES = 4, SL_MIN_TAPS = 3, SL_MAX_TAPS = 17;   // the filter cascade; taps = filter order + 1
constexpr int64_t SL_NT_MAX = 65536;                                  // samples of a discretised source-time function
struct SlStage {
    double b[SL_MAX_TAPS], a[SL_MAX_TAPS];   // zero beyond ntaps; a[0] = 1
    int32_t ntaps, demean;
};
// nt [D], A [D, ntmax]: the half-sinusoid amplitudes of every duration (k_stf_table)
int launch_stf_table(beatamd_ctx *ctx, int64_t D, const double *durations, double deltat, int64_t ntmax, int32_t *nt, double *A);
// Y [T * pb * D, Lcmax] = the responses X [T, P, L] of the patches [p0, p0 + pb) convolved with the rows of A (k_stf_convolve)
int launch_stf_convolve(beatamd_ctx *ctx, int64_t T, int64_t P, int64_t p0, int64_t pb, int64_t L, const double *X, int64_t D,
                        int64_t ntmax, const int32_t *nt, const double *A, int64_t Lcmax, double *Y);
// one filter stage over the first L + nt[q % D] - 1 samples of every row of Y [Q, Lcmax], in place (k_trace_filter)
int launch_trace_filter(beatamd_ctx *ctx, int64_t Q, int64_t D, int64_t L, int64_t ntmax, const int32_t *nt, int64_t Lcmax,
                        const SlStage &st, double *Y);
// lib [T, P, D, S, N], patches [p0, p0 + pb): the windows i0 [T, P, S] of the rows of Y, sample 0 times w0 [T, P, S]
int launch_library_windows(beatamd_ctx *ctx, int64_t T, int64_t P, int64_t p0, int64_t pb, int64_t D, int64_t L, int64_t ntmax,
                           const int32_t *nt, int64_t Lcmax, const double *Y, int64_t S, int64_t N, const int64_t *i0,
                           const double *w0, double *lib);

}  // namespace beatamd
