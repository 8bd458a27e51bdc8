// ctx.hpp -- context, error handling, host/device argument staging, kernel timing.
// Internal to libbeat_amd.so (gfx950 only; no CUDA/portability layer).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/beat_amd.h"

struct beatamd_ctx;

namespace beatamd {

void set_error(const char *fmt, ...);

#define BA_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            beatamd::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,                 \
                               hipGetErrorString(e_));                                       \
            return BEATAMD_EHIP;                                                             \
        }                                                                                    \
    } while (0)

#define BA_CHECK(cond, code, ...)                                                            \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            beatamd::set_error(__VA_ARGS__);                                                 \
            return (code);                                                                   \
        }                                                                                    \
    } while (0)

#define BA_TRY(expr)                                                                         \
    do {                                                                                     \
        int rc_ = (expr);                                                                    \
        if (rc_ != BEATAMD_OK) return rc_;                                                   \
    } while (0)

// device status bits set by kernels (checked at synchronisation points)
enum : int { ST_INDEX_OOB = 1, ST_BAD_HYPO = 2, ST_NOT_PSD = 4, ST_BAD_COV = 8, ST_BAD_SCALE = 16, ST_LINE_OOB = 32,
              ST_LINE_NONFINITE = 64, ST_SPAN_BAD = 128, ST_SPAN_OOB = 256 };

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes);
    void release();
};

// src -> dst on the context's stream (hipMemcpyDefault: either side may be host or device), synchronised
int dev_copy_sync(beatamd_ctx *ctx, void *dst, const void *src, size_t bytes);

// One hipMalloc'd array with an owner: freed when the owner goes (object destroyed, context closed, builder left early).
// Move-only.  Kernels and call structs get the plain pointer (get()).
template <class T>
class DevMem {
    T *p_ = nullptr;

public:
    DevMem() = default;
    DevMem(DevMem &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevMem &operator=(DevMem &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ~DevMem() { reset(); }
    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    // n elements, uninitialised (what was held is freed first); the caller words the error
    hipError_t try_alloc(size_t n)
    {
        reset();
        const hipError_t e = hipMalloc((void **)&p_, n ? n * sizeof(T) : 8);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p_ = nullptr;
        }
        return e;
    }
    int alloc(size_t n)
    {
        const hipError_t e = try_alloc(n);
        BA_CHECK(e == hipSuccess, BEATAMD_ENOMEM, "hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e));
        return BEATAMD_OK;
    }
    // n elements holding a copy of src (host or device memory; nullptr: uninitialised)
    int alloc_copy(beatamd_ctx *ctx, const T *src, size_t n)
    {
        BA_TRY(alloc(n));
        if (!src || !n) return BEATAMD_OK;
        const int rc = dev_copy_sync(ctx, p_, src, n * sizeof(T));
        if (rc != BEATAMD_OK) reset();
        return rc;
    }
};

struct SeisLib {
    int64_t T = 0, P = 0, D = 0, S = 0, N = 0;
    // target count the patch-range rule sees (gf_plan_call): 0 = T; the whole wavemap's T for a rank's block of targets
    int64_t split_T = 0;
    double st_min = 0, st_dt = 1, du_min = 0, du_dt = 1;
    double *g = nullptr;  // HBM, (T,P,D,S,N) C-order, N fastest
    float *g32 = nullptr; // optional float copy of g (beatamd_seis_gflib_round_to_f32; g then holds float-representable values)
    int64_t elems() const { return T * P * D * S * N; }
};

// a library as the context keeps it.  SeisLib itself stays a copyable view: the patch-range split stacks through
// re-shaped copies of it (launch_gfstack_split)
struct SeisStore : SeisLib {
    DevMem<double> own;    // behind g; empty while the storage is the caller's (beatamd_seis_gflib_adopt)
    DevMem<float> own32;   // behind g32
};

struct GeoLib {
    int64_t P = 0, Nobs = 0;
    DevMem<double> g;  // (P, Nobs)
};

// the libraries of the crust-model variants of one geodetic composite (geodetic.py:1161-1176): K variants of nvar slip
// variables, all of one shape.  The ensemble owns no library: it names them (ids, variant-major) and keeps the table of
// their device pointers that k_crust_stack reads; a stack on an ensemble whose library went or was replaced is refused
struct GeoEnsemble {
    int64_t K = 0, nvar = 0, P = 0, Nobs = 0;
    std::vector<int32_t> libs;              // [K * nvar]
    std::vector<const double *> ptrs;       // the libraries' storage when the table was written
    DevMem<const double *> table;           // device [K * nvar]
};

struct WeightSet {
    int kind = BEATAMD_W_SCALAR;
    int64_t nd = 0, M = 0;
    DevMem<double> w;     // [nd] or [nd,M,M]
    DevMem<double> slog;  // [nd]
    int upper_tri = 0;       // dense only: exact zeros below the diagonal in every W
    // dense only: every W is upper-triangular AND banded -- no entry further than `band` columns right of the diagonal
    // exceeds 2^-40 of the largest entry of its matrix (-1: not banded / band > QF_BAND_MAX).  The whitening operator of
    // the reference's "exponential" noise structure (covariance.py:24-51: C_ij = exp(-|i-j| dt / t0), a Markov kernel) is
    // bidiagonal: band = 1.  wb [nd, M, band + 1]: row i = W[i, i .. i+band] (k_quadform_banded)
    int64_t band = -1;
    DevMem<double> wb;
    double dropped_rel = 0.0;   // banded: the largest entry beyond the band, relative to the largest of its row (<= 2^-40)
};

struct Laplacian {
    int64_t P = 0;
    DevMem<double> L;
    double logdet = 0;
};

struct Wavemap {
    std::vector<int32_t> libs;
    DevMem<double> data;  // [T,N]
    int32_t wset = -1;
    DevMem<int64_t> hp_off;     // device [T]
    DevMem<int64_t> shift_off;  // device [T] or empty
    // targets that share a station correction (the channels of a station: heart.py:2941-2950 repeats the station
    // indices per channel) have the same start times -> the index tables are built per SLOT = distinct shift variable
    int32_t nslot = 0;             // 0: no shifts, or every target has its own (tables per target)
    DevMem<int32_t> tslot;         // device [T]: slot of target t
    DevMem<int64_t> slot_shift_off;      // device [nslot]: the shift variable of the slot
    int interp = 0;
    int64_t T = 0, N = 0;
    bool f32 = false;   // read the libraries' float copies where a kernel supports it
    // spectrum domain (beatamd_ffi_model_add_wavemap_spectrum; spectrum.hip): the likelihood is formed on the amplitude
    // spectra abs(rfft(., ntrans))[lo:hi] of the stacked traces, M = hi - lo samples per dataset; data_spec [T,M] is the
    // observed side and `data` stays empty (the entry point takes the observed spectra alone)
    int domain = BEATAMD_DOMAIN_TIME;
    int64_t ntrans = 0, lo = 0, hi = 0, M = 0;
    DevMem<double> data_spec;
    int64_t nsamples() const { return domain == BEATAMD_DOMAIN_SPECTRUM ? M : N; }   // samples per dataset in the likelihood
};

// one correction term of a geodetic dataset (geodetic.py:411-427 apply_corrections; corrections.py:46-87 ramp,
// :143-205 strain rate): corr[c,i] = sum_k B[i,k] * coef_k over the dataset's observations [start, start + n),
// coef_k = q[c, off[k]] or, with off[k] < 0, fix[k].  The table lives in device memory; the residual kernels read it
// through wave-uniform (scalar) loads
constexpr int GEO_CORR_MAX = 32;   // terms per composite (beatamd_ffi_model_add_geodetic_corrections)
//
// kind 1, the Euler pole (corrections.py:90-140, heart.py:4326-4392): K = 3 and the coefficients are not entries of q
// but omega' p, derived per chain from q[off[0..2]] = (pole_lat, pole_lon, omega) by k_pole_coef (corrections.hip) into
// the composite's record buffer pole [C, npole, 4] (32-byte records; slot 3 is zero).  `rec` is the term's record
struct GeoCorrTerm {
    int64_t start, n;
    const double *B;      // device [K, n]: column k at B + k*n
    int64_t off[4];
    double fix[4];
    int32_t K, kind;      // kind: GEO_CORR_LINEAR / GEO_CORR_POLE
    int32_t rec, pad_;    // kind 1: index of the term's record within a chain's records
};
constexpr int GEO_CORR_LINEAR = 0, GEO_CORR_POLE = 1;
// what k_pole_coef reads per pole term: the slots of (pole_lat, pole_lon, omega) [deg, deg, deg/Myr] in q (-1: fix)
// and the earth's (radius, equatorial radius, oblateness)
struct PoleTerm {
    int64_t off[3];
    double fix[3];
    double earth[3];
};
struct GeoCorr {
    const GeoCorrTerm *terms = nullptr;   // device [nterm]
    int32_t nterm = 0;
    int32_t npole = 0;                    // pole terms among them
    const double *pole = nullptr;         // device [C, npole, 4]: the derived coefficients, written by k_pole_coef
    int64_t pole_stride = 0;              // doubles per chain: npole * 4
    const PoleTerm *pole_terms = nullptr; // device [npole]
};

struct Geodetic {
    std::vector<int32_t> libs;
    DevMem<double> data, odws;  // [Nobs]
    int64_t Nobs = 0;
    std::vector<int64_t> sizes;
    std::vector<int32_t> wsets;
    DevMem<int64_t> hp_off;  // device [nd]
    // dataset corrections (hierarchical parameters), in the order they are subtracted
    bool corr_set = false;
    GeoCorr corr;                        // what the kernels get: a view of corr_terms
    DevMem<GeoCorrTerm> corr_terms;      // device [corr.nterm]
    DevMem<double> corr_basis;           // device, the terms' basis columns concatenated
    // pole terms: their inputs, and the derived-coefficient records of pole_chains chains.  Allocated with the table and
    // grown with the chain count by geo_pole_coefficients (model.cpp), never inside a graph capture
    DevMem<PoleTerm> pole_terms;         // device [corr.npole]
    mutable DevMem<double> pole_coef;    // device [pole_chains, corr.npole, 4] (a cache of the evaluator, hence mutable)
    mutable int64_t pole_chains = 0;
};

// geometry-mode sources of the geodetic composite (analytic half space)
struct GeomSources {
    int nsrc = 0;
    DevMem<int32_t> kind;   // device [nsrc]
    DevMem<int64_t> poff;   // device [nsrc*10]
    DevMem<double> pfix;    // device [nsrc*10]
    DevMem<double> east, north, los;  // device [Nobs], [Nobs], [Nobs,3]
    int64_t Nobs = 0;
    double nu = 0.25;
};

// the polarity composite (polarity.hip; beat/models/polarity.py): one point source, nmap polarity maps whose stations
// stand side by side in rw / obs.  Source slot k is q[off[k]] or, with off[k] < 0, fix[k] (the convention of GeomSources)
constexpr int POL_MTQT = 0, POL_MT = 1, POL_DC = 2;
constexpr int POL_MAX_MAPS = 8;
struct PolSource {
    int32_t kind = POL_MTQT, pad_ = 0;
    int64_t off[6] = {-1, -1, -1, -1, -1, -1};
    double fix[6] = {0, 0, 0, 0, 0, 0};
};
struct Polarity {
    PolSource src;
    int32_t nmap = 0;
    int64_t NT = 0;                              // stations of all maps
    int64_t map_end[POL_MAX_MAPS] = {};          // exclusive end of every map's stations
    int64_t hp_off[POL_MAX_MAPS] = {};           // the map's sigma in q, or -1: hp_fix
    double hp_fix[POL_MAX_MAPS] = {};
    double gamma = 0.2;
    DevMem<double> rw, obs;                      // device [6, NT], [NT]
    int32_t ntab = 0;
    DevMem<double> utab, btab;                   // device [ntab]: U_MAPPING, BETA_MAPPING (mtqt only)
};

struct FfiModel {
    beatamd_ffi_layout layout;
    int32_t nsub = 0;
    std::vector<int32_t> ndip, nstrike, patch_off;
    std::vector<double> patch_size;
    int64_t P = 0;
    DevMem<int32_t> d_ndip, d_nstrike, d_patch_off;
    DevMem<double> d_patch_size;
    std::vector<Wavemap> wavemaps;
    bool has_geo = false;
    Geodetic geo;
    bool geo_is_geometry = false;  // mu from analytic sources instead of G.T . slips
    GeomSources geom;
    bool has_pol = false;
    Polarity pol;
    int32_t lap = -1;
    int64_t nllk() const;
    // |W_k d_k|^2 of every dataset (beatamd_ffi_obs_quads), computed on first use and kept until the weights, the data
    // or the corrections of the model change: host copy and the device copy the variance-reduction kernel reads
    bool obs_quads_valid = false;
    std::vector<double> obs_quads;
    DevMem<double> d_obs_quads;
    // lsq start (lsq.hip): which slip variable is inverted and which is set to zero (indices into layout.slip_off, -1:
    // none), and the chain-independent blocks G_v G_v^T and L^T L [P, P] (lower triangles), formed on first use and kept
    // until the model's data, corrections or laplacian are replaced
    int32_t lsq_var = -1, lsq_zero_var = -1;
    bool lsq_blocks_valid = false;
    DevMem<double> lsq_GG, lsq_LtL;
};

// the hyper-parameter model (hyper.hip): term k = kind[k] formula on hyper-parameter hp_index[k] of the nh-vector
struct HyperModel {
    int64_t nterm = 0, nh = 0;
    DevMem<double> M, slog;          // device [nterm]
    DevMem<int32_t> kind, hp_index;  // device [nterm]
    int32_t ngroups = 0, group_end[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // composites inside the term vector (exclusive ends)
};

// A/B and test knobs of the stacking path (BEATAMD_G* / BEATAMD_WS_* environment variables; DESIGN.md 3.1b lists them).
// Read ONCE when the context is created (and again on beatamd_ctx_reload_knobs); a context created with
// BEATAMD_KNOBS_LIVE=1 in the environment -- the test suite, the A/B tools -- re-reads them at every stacking call so
// that one process can compare kernels.  KNOB_UNSET: the variable is not set, the default applies.
constexpr int KNOB_UNSET = -2147483647;
// Stated once: X(member, environment variable) -> the fields of GfKnobs and GfKnobs::read_env
#define BEATAMD_GF_KNOBS(X) \
    X(gf_kernel, "BEATAMD_GF_KERNEL") X(gs_cg, "BEATAMD_GS_CG") X(gs_ws, "BEATAMD_GS_WS") X(gs_dma, "BEATAMD_GS_DMA") X(gs_nt, "BEATAMD_GS_NT") \
    X(ws_map, "BEATAMD_WS_MAP") X(gs_pair, "BEATAMD_GS_PAIR") X(gs_nthint, "BEATAMD_GS_NTHINT") X(gs_order, "BEATAMD_GS_ORDER") \
    X(gs_fit, "BEATAMD_GS_FIT") X(gs_win, "BEATAMD_GS_WIN") X(gf_tinv, "BEATAMD_GF_TINV") X(gs_tune, "BEATAMD_GS_TUNE") \
    X(gf_order, "BEATAMD_GF_ORDER") X(gf_cgroup, "BEATAMD_GF_CGROUP") X(gs_ml, "BEATAMD_GS_ML") X(gc_global, "BEATAMD_GC_GLOBAL") \
    X(gc_sort, "BEATAMD_GC_SORT") X(gc_keys, "BEATAMD_GC_KEYS") X(gc_bands, "BEATAMD_GC_BANDS") X(gr_cap, "BEATAMD_GR_CAP") \
    X(gr_pass_alloc, "BEATAMD_GR_PASS_ALLOC") X(gr_var, "BEATAMD_GR_VAR") X(sweep_v1, "BEATAMD_SWEEP_V1") X(qf_band, "BEATAMD_QF_BAND") \
    X(qf_fuse, "BEATAMD_QF_FUSE") X(gf_split, "BEATAMD_GF_SPLIT") X(gm_wave, "BEATAMD_GM_WAVE") X(skip_parked, "BEATAMD_SKIP_PARKED") \
    X(td_strip, "BEATAMD_TD_STRIP") X(pd_strip, "BEATAMD_PD_STRIP") X(pd_rows, "BEATAMD_PD_ROWS")
struct GfKnobs {
#define X(member, env) int member = KNOB_UNSET;
    BEATAMD_GF_KNOBS(X)
#undef X
    void read_env();
    static int get(int v, int dflt) { return v == KNOB_UNSET ? dflt : v; }
    static bool is(int v, int x) { return v != KNOB_UNSET && v == x; }       // set and equal to x
    static bool set(int v) { return v != KNOB_UNSET; }
};

struct KTimer {
    double total_ms = 0;
    int64_t n = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

}  // namespace beatamd

struct beatamd_ctx {
    int device = 0;
    hipStream_t stream = nullptr, own_stream = nullptr;
    bool timing = false;
    std::map<std::string, beatamd::KTimer> timers;
    std::vector<hipEvent_t> event_pool;
    int *d_status = nullptr;  // device status word
    std::vector<beatamd::DevBuf> scratch_bufs;
    std::vector<std::unique_ptr<beatamd::SeisStore>> seislibs;
    std::vector<std::unique_ptr<beatamd::GeoLib>> geolibs;
    std::vector<std::unique_ptr<beatamd::GeoEnsemble>> geoens;
    std::vector<std::unique_ptr<beatamd::WeightSet>> wsets;
    std::vector<std::unique_ptr<beatamd::Laplacian>> laps;
    std::vector<std::unique_ptr<beatamd::FfiModel>> models;
    std::vector<std::unique_ptr<beatamd::HyperModel>> hypers;
    int num_cu = 256;
    // name of the stacking kernel of the most recent launch (tests assert which kernel ran)
    char last_gf_kernel[96] = "";
    // distinct-row statistics of the most recent chain-shared launch (bench.py roofline leg)
    int64_t gs_ngtp = 0, gs_N = 0;
    double gs_trep = 1;             // targets served by one table cell (T / table slots)
    int gs_nvar = 1;                // slip variables: every distinct row is staged once per variable
    bool gs_has_passes = false;     // the statistics slot holds [rows per patch][passes per patch]
    // what the selection chose for the most recent stacking launch and why (beatamd_ctx_gf_plan)
    char gf_plan[384] = "";
    char gf_tune_log[512] = "";   // the most recent group-size measurement (launch_gfstack), in words
    // largest distinct-row count of the previous small-group launch, read back asynchronously
    // (pinned mailbox + event; never waited for): sizes the next launch's row buffers
    uint32_t *h_umax = nullptr;
    hipEvent_t umax_event = nullptr;
    bool umax_pending = false;
    int umax_hist = -1, umax_hist_cg = 0;
    // measured chains-per-workgroup choice per problem shape: key -> (group size, row bound)
    std::map<std::vector<int64_t>, std::pair<int, int>> gs_tuned;
    int gs_cg = 0;
    beatamd::GfKnobs knobs;
    bool knobs_live = false;
    // device-resident Philox step counter (beatamd_ctx_set_step_counter): the proposal draws read it
    // instead of their `step` argument and advance it, so that a captured step replays correctly
    uint32_t *step_dev = nullptr;
    // twiddle tables of the amplitude-spectrum kernel, one per transform length (spectrum.hip: spectrum_twiddles)
    std::map<int64_t, beatamd::DevMem<double>> twiddles;

    // grow-only scratch slot
    int get_scratch(int slot, size_t bytes, void **out);
    // the slot as n elements of T
    template <class T>
    int scratch(int slot, size_t n, T **out)
    {
        void *raw = nullptr;
        const int rc = get_scratch(slot, n * sizeof(T), &raw);
        *out = static_cast<T *>(raw);
        return rc;
    }
    hipEvent_t get_event();
    void time_begin(const char *name);
    void time_end(const char *name);
    int check_status();  // sync + read status word; maps to BEATAMD_E*
};

namespace beatamd {

bool is_device_ptr(const void *p);
// the knobs in force for a stacking call (re-read from the environment first in live mode)
const GfKnobs &gf_knobs(beatamd_ctx *ctx);

// scratch slot map (one per logical temporary so slots never alias within a call)
enum Slot : int {
    SL_IN0 = 0, SL_IN1, SL_IN2, SL_IN3, SL_IN4, SL_IN5, SL_IN6, SL_IN7,
    SL_OUT0, SL_OUT1, SL_OUT2, SL_OUT3, SL_OUT4, SL_OUT5, SL_OUT6, SL_OUT7,
    SL_ROWOFF, SL_WEIGHTS, SL_ST0, SL_RESID, SL_PARTIAL, SL_PARTIAL2, SL_QUAD, SL_MU, SL_SLIPS,
    SL_QPROP, SL_LPROP, SL_MISC, SL_GS_UROWS, SL_GS_UCOUNT, SL_GS_SLOT, SL_GS_W, SL_GS_UMAX, SL_GS_USLOT,
    SL_CHAINBAD, SL_Z, SL_ROWSCALE, SL_CUM, SL_STAGE2, SL_WHITEN,
    SL_CHOL_A, SL_CHOL_X, SL_CHOL_D, SL_CHOL_T, SL_CHOL_L,
    SL_GC_ORDER, SL_GS_ORDER, SL_GC_STREAM, SL_GC_HDR, SL_GC_META, SL_DELTA, SL_LOGU, SL_EDGES, SL_TSLOT, SL_SPLIT, SL_WS_PACK,
    SL_GM_W, SL_GM_SCALE, SL_GM_FLAG, SL_LSQ_N, SL_LSQ_B, SL_LSQ_X, SL_LSQ_U, SL_MR_SPANS,
    SL_RES_GG, SL_RES_N, SL_RES_W, SL_RES_T, SL_RES_U, SL_RATE_DMIN, SL_SPEC,
    SL_MG_FLAG, SL_MG_MOM, SL_MG_PAR, SL_MG_GRID, SL_MG_W, SL_MG_BOX,
    SL_MC_FLAG, SL_MC_COUNT, SL_MC_SUM, SL_PD_BOX,
    SL_CV_W, SL_CV_SA, SL_CV_SB, SL_CV_Q, SL_CV_CM, SL_CV_RM, SL_CV_OFF, SL_CV_ESS, SL_CV_ACT, SL_CV_STATE, SL_CV_MAC0, SL_CV_MAC1,
    SL_CV_AC, SL_CV_RHO, SL_CV_PART, SL_COUNT
};
constexpr int SL_NIN = SL_OUT0 - SL_IN0, SL_NOUT = SL_ROWOFF - SL_OUT0;   // the slots of Staging

// The array arguments of one entry point.  An argument may live on either side: NULL, an empty array and a device pointer
// pass through; a host array is mirrored in a scratch slot (SL_IN* / SL_OUT*, handed out in call order) -- inputs go up
// on the context's stream, outputs come back in finish().
class Staging {
    beatamd_ctx *ctx;
    int nin = 0, nout = 0, nback = 0;
    struct { void *host, *dev; size_t bytes; } back[SL_NOUT];   // host outputs: copied back by finish()
    int in_bytes(const void *p, size_t bytes, const void **dev);
    int out_bytes(void *p, size_t bytes, void **dev, bool preload);

public:
    explicit Staging(beatamd_ctx *c) : ctx(c) {}
    // *dev: device pointer that holds the n elements of p
    template <class T>
    int in(const T *p, size_t n, const T **dev)
    {
        const void *d = nullptr;
        BA_TRY(in_bytes(p, n * sizeof(T), &d));
        *dev = static_cast<const T *>(d);
        return BEATAMD_OK;
    }
    // *dev: device pointer to write the n elements into; preload: a host array's present content goes up first
    template <class T>
    int out(T *p, size_t n, T **dev, bool preload = false)
    {
        void *d = nullptr;
        BA_TRY(out_bytes(p, n * sizeof(T), &d, preload));
        *dev = static_cast<T *>(d);
        return BEATAMD_OK;
    }
    // D2H copies; synchronises and reads the status word iff some output was a host array
    int finish();
};

struct ScopedTimer {
    beatamd_ctx *c;
    const char *n;
    ScopedTimer(beatamd_ctx *ctx, const char *name) : c(ctx), n(name) { c->time_begin(n); }
    ~ScopedTimer() { c->time_end(n); }
};

}  // namespace beatamd
