// sweep.hip -- batched eikonal fast sweeping (rupture onset times) for gfx950.
//
// Reference arithmetic: beat/fast_sweeping/fast_sweep_ext.c:65-206 (eq_solve, upwind,
// fast_sweep).  One 64-lane wavefront owns one (chain, subfault) grid held in LDS.
//
// The reference runs 4 sequential Gauss-Seidel sweeps per outer iteration.  A cell (i,j)
// of a sweep reads the already-updated upwind neighbours (i-1,j),(i,j-1) and the
// not-yet-updated downwind neighbours (in sweep order).  Cells on one anti-diagonal
// i'+j' = k of the sweep-ordered grid neither read nor write each other, and all their
// upwind inputs lie on diagonal k-1, so processing diagonals in order k = 0..ni+nj-2 with
// the lanes spread along the diagonal performs EXACTLY the same double operations on the
// same operands as the sequential loop: results are bitwise those of a sequential
// implementation of the same expressions.  (The reference's glibc pow(x,0.5) is replaced
// by the correctly rounded sqrt; times agree to ~1 ulp)
//
// Built with -ffp-contract=off: no FMA contraction, the C expression order is kept.
#include "kernels.hpp"
#include "wave.hpp"

namespace beatamd {

// fast_sweep_ext.c:65-75
__device__ __forceinline__ double eq_solve(double a, double b, double f, double h)
{
    double v;
    if (fabs(a - b) >= f * h) {
        v = (a < b) ? a : b;
        v += f * h;
    } else {
        double dab = a - b;
        v = a + b + sqrt(2.0 * f * f * h * h - dab * dab);
        v /= 2.0;
    }
    return v;
}

// fast_sweep_ext.c:77-118
__device__ __forceinline__ double upwind(const double *t, int i, int j, const double *slow,
                                         double h, int ni, int nj)
{
    int i1 = i - 1, i2 = i + 1, j1 = j - 1, j2 = j + 1;
    if (i1 < 0) i1 = 0;
    if (i2 >= ni) i2 = ni - 1;
    if (j1 < 0) j1 = 0;
    if (j2 >= nj) j2 = nj - 1;
    double a1 = t[i1 * nj + j], a2 = t[i2 * nj + j];
    double b1 = t[i * nj + j1], b2 = t[i * nj + j2];
    double old = t[i * nj + j];
    double uxmin = (a1 < a2) ? a1 : a2;
    double uymin = (b1 < b2) ? b1 : b2;
    double v = eq_solve(uxmin, uymin, slow[i * nj + j], h);
    return (v < old) ? v : old;
}

// v_min_f64 / v_med3_i32 by name: the compiler keeps compare + two selects for `(a < b) ? a : b` (its NaN rule differs
// from the instruction's) and forms the integer median only from constant bounds.
__device__ __forceinline__ double min_f64(double a, double b)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ int med3_i32(int x, int a, int b)
{
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(a), "v"(b));
    return r;
}

// lane l receives x of lane l - 1, lane 0 receives own (DPP wave_shr:1 leaves the destination of a lane without a source
// as it was).  Must run with every lane of the wavefront enabled.
__device__ __forceinline__ double from_lane_below_or(double own, double x)
{
    int lo = __builtin_amdgcn_update_dpp(__double2loint(own), __double2loint(x), 0x138, 0xf, 0xf, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(own), __double2hiint(x), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// sqrt(x) for 0x1p-767 <= x < inf: the Newton core of the compiler's correctly rounded f64 sqrt without its range scaling
// (x < 0x1p-767 only) and its class fix-up (x = +-0, +inf only), both idle on this interval -- the same instructions on
// the same x, so the same bits.  x < 0 and NaN give NaN in both; +inf gives NaN here and +inf there (see SWEEP_PLAIN).
__device__ __forceinline__ double sqrt_unscaled(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}

// The slowness terms of eq_solve, S = f*h and S2 = 2*f*f*h*h, formed once per grid (same expressions, same values as the
// first version forms per visit) and kept as one 16-byte LDS record per cell.
struct __attribute__((aligned(16))) SlowTerms {
    double S, S2;
};

// SWEEP_PLAIN: a cell passes when S2 - S*S >= 0x1p-767 (false for NaN).  eq_solve takes its sqrt arm only where
// |a - b| < S, so there (a-b)*(a-b) <= S*S after rounding (rounding is monotone) and the sqrt argument S2 - (a-b)*(a-b)
// is >= S2 - S*S >= 0x1p-767: sqrt_unscaled applies unless the argument is +inf (S2 overflowed, S did not).  Then the
// arm's value is +inf with sqrt and NaN with sqrt_unscaled, and the closing min(v, old) returns old for both.  The value
// of the arm that is not selected never reaches a result.  Grids with a cell that fails use sqrt().
__device__ __forceinline__ bool put_terms(SlowTerms *p, double f, double h)
{
    SlowTerms w;
    w.S = f * h;
    w.S2 = 2.0 * f * f * h * h;
    *p = w;
    return w.S2 - w.S * w.S >= 0x1p-767;
}

// One sweep of fast_sweep_ext.c:141-196 by anti-diagonals for grids of at most 64 rows.  In sweep order lane ip owns row
// ip and walks it one cell per diagonal: the upwind neighbour in its own row, (ip, jp-1), is the value the lane computed
// on the previous diagonal (a register), the upwind neighbour in the row below, (ip-1, jp), is what lane ip-1 computed on
// the previous diagonal (one DPP move).  The cell's old value, its downwind row neighbour (diagonal d+1: not written yet in
// this sweep) and its slowness terms do not depend on anything this sweep has written before diagonal d+1 and are read
// from LDS TWO diagonals ahead; the downwind neighbour in the own row, (ip, jp+1), IS the old value of the next diagonal's
// cell.  Same operands, same operations, same order per cell as the first version (sweep_wave's LDS loop): bitwise the same
// times.
//
// What a diagonal costs is its instruction count (a wavefront alone on its SIMD issues one instruction per ~4 cycles
// whatever it computes), so:
//  * a lane's cell is ONE clamped index: x, the cell index of (ip, d - ip) counted along the row as if the row had no
//    ends, advances by sj = +-1 per diagonal; kc = med3(x, kbeg, kend) is the cell the reference's clamp rule reads (before
//    the row: its first cell, whose old value is what a first cell takes for its missing upwind neighbour; beyond the
//    row: the last cell, read before it is written, i.e. the own old value the reference clamps to); the lane is on the
//    grid exactly when the clamp left x alone.  Lanes without a row hold an x that never meets the grid.
//  * the minima are v_min_f64.  Times are +0, positive or +inf, never NaN (the closing min keeps old when v is NaN, and
//    old starts at +inf or 0) and never -0, so min(a1, a2) is the value of (a1 < a2) ? a1 : a2 in either operand order,
//    and the direction of the sweep leaves the instructions alone.  The closing (v < old) ? v : old sees a quiet NaN v
//    (inf - inf, sqrt of a negative) and must return old: v_min_f64 returns the operand that is not NaN.  The choice
//    between the arms of eq_solve stays a compare and select: fabs(dab) >= S is false for a NaN dab.
//  * three diagonals per trip: the values fetched ahead rotate by renaming.  Trips run past the last diagonal (at most
//    two steps): every lane is off the grid there, nothing is stored.
//  * vprev is the lane's previous result while it is on the grid and the old value of the NEXT diagonal's cell while it is
//    not, which is what a first cell takes for (ip, -1).
template <bool PLAIN>
__device__ __forceinline__ void sweep_diag64(double *t, const SlowTerms *terms, int ni, int nj, bool irev, bool jrev,
                                              int lane)
{
    const bool row = lane < ni;
    const int i = row ? (irev ? ni - 1 - lane : lane) : 0;
    // true row of sweep row ip + 1; beyond the grid the reference clamps to the cell's own row (its old value)
    const int idn = (lane + 1 < ni) ? (irev ? i - 1 : i + 1) : i;
    const int sj = jrev ? -1 : 1;
    const int kbeg = i * nj + (jrev ? nj - 1 : 0), kend = i * nj + (jrev ? 0 : nj - 1);
    const int kdn = (idn - i) * nj;
    int x = row ? kbeg - sj * lane : -sj * (1 << 24);

    double O0, O1, O2, D0, D1, D2;
    SlowTerms P0, P1, P2;
    int k0, k1, k2;
    bool on0, on1, on2;
    auto fetch = [&](int xd, int &k, bool &on, double &o, double &dn, SlowTerms &p) {
        k = med3_i32(xd, kbeg, kend);
        on = k == xd;
        o = t[k];
        dn = t[k + kdn];
        p = terms[k];
    };
    double vprev;
    // diagonal d: the cell k (old value o, row neighbour dn, terms p), onext the old value of diagonal d + 1's cell
    auto cell = [&](int k, bool on, double o, double onext, double dn, const SlowTerms &p) {
        const double ui = from_lane_below_or(o, vprev);     // (ip-1, jp) of this sweep; sweep row 0: the own old value
        // fast_sweep_ext.c:77-118 upwind(): uxmin over t[i-1][j], t[i+1][j]; uymin over t[i][j-1], t[i][j+1]
        const double uxmin = min_f64(ui, dn);
        const double uymin = min_f64(vprev, onext);
        // eq_solve (fast_sweep_ext.c:65-75), both arms evaluated and selected
        const double dab = uxmin - uymin;
        const double vlin = min_f64(uxmin, uymin) + p.S;
        const double q = p.S2 - dab * dab;
        const double vsq = (uxmin + uymin + (PLAIN ? sqrt_unscaled(q) : sqrt(q))) / 2.0;
        double v = (fabs(dab) >= p.S) ? vlin : vsq;
        v = min_f64(v, o);
        if (on) t[k] = v;
        vprev = on ? v : onext;
    };
    fetch(x, k0, on0, O0, D0, P0);
    fetch(x + sj, k1, on1, O1, D1, P1);
    x += 2 * sj;
    vprev = O0;
    for (int d = 0; d < ni + nj - 1; d += 3) {
        fetch(x, k2, on2, O2, D2, P2);
        cell(k0, on0, O0, O1, D0, P0);
        fetch(x + sj, k0, on0, O0, D0, P0);
        cell(k1, on1, O1, O2, D1, P1);
        fetch(x + 2 * sj, k1, on1, O1, D1, P1);
        cell(k2, on2, O2, O0, D2, P2);
        x += 3 * sj;
    }
}

// fast_sweep_ext.c:120-206, one wavefront.  t/told/slow are this wave's LDS arrays; a grid of at most 64 rows that does
// not ask for the first version has its slowness as terms (plain: SWEEP_PLAIN holds for every cell) and no slow.
// (Inlined into the kernel: as a call its arguments are generic pointers and per-lane integers, and the loops lose their
// LDS instructions and their scalar counters.)
__device__ __forceinline__ void sweep_wave(double *t, double *told, const double *slow, const SlowTerms *terms, bool plain, int ni,
                           int nj, double h, int hi, int hj, int lane, bool a_first_version)
{
    const int n = ni * nj;
    for (int k = lane; k < n; k += 64) t[k] = __builtin_inf();
    wave_lds_sync();
    if (lane == 0) t[hi * nj + hj] = 0.0;
    wave_lds_sync();

    double err = 1.0e6;
    int iter = 0;
    while (err > 0.1) {
        for (int k = lane; k < n; k += 64) told[k] = t[k];
        wave_lds_sync();
        for (int sw = 0; sw < 4; sw++) {
            const bool irev = (sw == 1) || (sw == 2);
            const bool jrev = (sw == 2) || (sw == 3);
            if (ni <= 64 && !a_first_version) {
                if (plain)
                    sweep_diag64<true>(t, terms, ni, nj, irev, jrev, lane);
                else
                    sweep_diag64<false>(t, terms, ni, nj, irev, jrev, lane);
                wave_lds_sync();
                continue;
            }
            for (int d = 0; d < ni + nj - 1; d++) {
                for (int base = 0; base < ni; base += 64) {
                    const int ip = base + lane;
                    const int jp = d - ip;
                    if (ip < ni && jp >= 0 && jp < nj) {
                        const int i = irev ? (ni - 1 - ip) : ip;
                        const int j = jrev ? (nj - 1 - jp) : jp;
                        const double v = upwind(t, i, j, slow, h, ni, nj);
                        t[i * nj + j] = v;
                    }
                }
                wave_lds_sync();
            }
        }
        // err = sum (new-old)^2  (fast_sweep_ext.c:199-202)
        double e = 0.0;
        for (int k = lane; k < n; k += 64) {
            double dlt = t[k] - told[k];
            e += dlt * dlt;
        }
        err = wave_butterfly<OpAdd>(e);
        if (fabs(err - 0.1) <= 1e-9) {
            // the decision is within reach of the summation order: redo the sum in the
            // reference's sequential order
            double es = 0.0;
            for (int k = 0; k < n; k++) {
                double dlt = t[k] - told[k];
                es += dlt * dlt;
            }
            err = es;
        }
        if (++iter >= 100000) break;  // the updates are monotone: never reached; bounds a hang
    }
}

struct SweepParams {
    int mode;  // 0: explicit slowness + integer hypocentres, 1: from the parameter matrix Q
    int64_t nprob;
    // mode 0
    const double *slow;
    const int32_t *hi, *hj;
    int32_t ni, nj;
    double h;
    // mode 1
    const double *Q;
    int64_t nparams, vel_off, nuc_strike_off, nuc_dip_off, time_off, P;
    const int32_t *sf_ndip, *sf_nstrike, *sf_off;
    const double *sf_h;
    int32_t nsub;
    // common
    double *out;
    int *status;
    int32_t *chain_bad;  // mode 1, nullable: chain flagged when its hypocentre index is off the grid
    int32_t nmax;  // LDS doubles reserved per array per wave
    int32_t first_version;   // BEATAMD_SWEEP_V1=1: the LDS-only diagonal loop also for grids of <= 64 rows (A/B, tests)
};

// LDS of one wavefront: t, told and a slowness area of nmax doubles each.  The slowness area is twice as large where that
// fits (SlowTerms records of grids of at most 64 rows; the first version uses its first half); larger subfaults keep the
// three arrays and run the first version.
constexpr int SWEEP_TERMS_MAX_CELLS = 5120;        // 4 arrays x 5120 x 8 B = 160 KiB, one wavefront per workgroup
constexpr size_t SWEEP_WG_LDS_DEFAULT = 64 * 1024;  // a launch may ask for this much dynamic LDS without opting in

__host__ __device__ inline int sweep_lds_arrays(int nmax) { return nmax <= SWEEP_TERMS_MAX_CELLS ? 4 : 3; }

// The launch shape of a batch whose largest subfault has nmax_cells patches: four grids per workgroup while their LDS
// stays within the default limit (nmax <= 512), else one.
SweepLdsPlan sweep_lds_plan(int nmax_cells)
{
    SweepLdsPlan pl;
    pl.nmax = (nmax_cells + 1) & ~1;
    const size_t per_wave = (size_t)sweep_lds_arrays(pl.nmax) * pl.nmax * sizeof(double);
    pl.waves = (4 * per_wave <= SWEEP_WG_LDS_DEFAULT) ? 4 : 1;
    pl.bytes = pl.waves * per_wave;
    return pl;
}

template <int WAVES>
__global__ void __launch_bounds__(WAVES * 64) k_fast_sweep(SweepParams a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    // (the wave number through readfirstlane: the grid's shape, its LDS addresses and the loop counts are then scalar)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t prob = (int64_t)blockIdx.x * WAVES + wave;
    if (prob >= a.nprob) return;
    const int arrays = sweep_lds_arrays(a.nmax);
    double *t = smem + (size_t)wave * arrays * a.nmax;
    double *told = t + a.nmax;
    double *slow = told + a.nmax;
    SlowTerms *terms = reinterpret_cast<SlowTerms *>(slow);
    const bool first_version = a.first_version != 0 || arrays < 4;
    bool plain = true;

    int ni, nj, hi, hj;
    double h, tadd = 0.0;
    double *out;
    if (a.mode == 0) {
        ni = a.ni;
        nj = a.nj;
        h = a.h;
        hi = a.hi[prob];
        hj = a.hj[prob];
        const double *s = a.slow + prob * (int64_t)(ni * nj);
        if (ni <= 64 && !first_version) {
            for (int k = lane; k < ni * nj; k += 64) plain &= put_terms(terms + k, s[k], h);
        } else {
            for (int k = lane; k < ni * nj; k += 64) slow[k] = s[k];
        }
        out = a.out + prob * (int64_t)(ni * nj);
    } else {
        const int64_t c = prob / a.nsub;
        const int sf = (int)(prob - c * a.nsub);
        ni = a.sf_ndip[sf];
        nj = a.sf_nstrike[sf];
        h = a.sf_h[sf];
        const double *q = a.Q + c * a.nparams;
        // utility.py:1542-1558 positions2idxs with cell = patch size, min_pos = 0
        // (ffi/fault.py:866-894): round-half-even -> rint, cast through int16
        const double pd = q[a.nuc_dip_off + sf], ps = q[a.nuc_strike_off + sf];
        hi = (int)(int16_t)(long long)rint((pd - 0.0 - (h / 2.0)) / h);
        hj = (int)(int16_t)(long long)rint((ps - 0.0 - (h / 2.0)) / h);
        tadd = q[a.time_off + sf];
        const double *v = q + a.vel_off + a.sf_off[sf];
        // seismic.py:1264: slowness = 1 / velocities
        if (ni <= 64 && !first_version) {
            for (int k = lane; k < ni * nj; k += 64) plain &= put_terms(terms + k, 1.0 / v[k], h);
        } else {
            for (int k = lane; k < ni * nj; k += 64) slow[k] = 1.0 / v[k];
        }
        out = a.out + c * a.P + a.sf_off[sf];
    }
    if (hi < 0 || hi >= ni || hj < 0 || hj >= nj) {
        // the reference writes outside its array here; we flag and clamp
        if (lane == 0) {
            atomicOr(a.status, ST_BAD_HYPO);
            if (a.mode == 1 && a.chain_bad) a.chain_bad[prob / a.nsub] = 1;
        }
        hi = min(max(hi, 0), ni - 1);
        hj = min(max(hj, 0), nj - 1);
    }
    wave_lds_sync();
    sweep_wave(t, told, slow, terms, __all(plain) != 0, ni, nj, h, hi, hj, lane, first_version);
    wave_lds_sync();
    // seismic.py:1268: starttimes_tmp += time[index]
    for (int k = lane; k < ni * nj; k += 64) out[k] = (a.mode == 0) ? t[k] : (t[k] + tadd);
}

static int launch_sweep(beatamd_ctx *ctx, SweepParams &p, int nmax_cells)
{
    BA_CHECK(nmax_cells > 0 && nmax_cells <= SWEEP_MAX_CELLS, BEATAMD_EINVAL,
             "fast sweep: subfault with %d patches exceeds the LDS-resident limit (%d)",
             nmax_cells, SWEEP_MAX_CELLS);
    const SweepLdsPlan pl = sweep_lds_plan(nmax_cells);
    p.nmax = pl.nmax;
    p.status = ctx->d_status;
    p.first_version = GfKnobs::get(gf_knobs(ctx).sweep_v1, 0) != 0 ? 1 : 0;     // (A/B: the round-3 kernel)
    ScopedTimer tm(ctx, "sweep");
    const size_t lds = pl.bytes;
    if (pl.waves == 4) {
        const int W = 4;
        unsigned grid = (unsigned)((p.nprob + W - 1) / W);
        hipLaunchKernelGGL(k_fast_sweep<4>, dim3(grid), dim3(W * 64), lds, ctx->stream, p);
    } else {
        if (lds > SWEEP_WG_LDS_DEFAULT)
            BA_HIP(hipFuncSetAttribute((const void *)k_fast_sweep<1>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_fast_sweep<1>, dim3((unsigned)p.nprob), dim3(64), lds, ctx->stream,
                           p);
    }
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

int launch_sweep_explicit(beatamd_ctx *ctx, const double *slow, double h, const int32_t *hi,
                          const int32_t *hj, int ni, int nj, int64_t C, double *out)
{
    SweepParams p;
    memset(&p, 0, sizeof(p));
    p.mode = 0;
    p.nprob = C;
    p.slow = slow;
    p.hi = hi;
    p.hj = hj;
    p.ni = ni;
    p.nj = nj;
    p.h = h;
    p.out = out;
    return launch_sweep(ctx, p, ni * nj);
}

int launch_sweep_model(beatamd_ctx *ctx, const FfiModel &m, const double *Q, int64_t C,
                       double *starttimes0, int32_t *chain_bad)
{
    SweepParams p;
    memset(&p, 0, sizeof(p));
    p.mode = 1;
    p.nprob = C * m.nsub;
    p.Q = Q;
    p.nparams = m.layout.nparams;
    p.vel_off = m.layout.velocities_off;
    p.nuc_strike_off = m.layout.nuc_strike_off;
    p.nuc_dip_off = m.layout.nuc_dip_off;
    p.time_off = m.layout.time_off;
    p.P = m.P;
    p.sf_ndip = m.d_ndip.get();
    p.sf_nstrike = m.d_nstrike.get();
    p.sf_off = m.d_patch_off.get();
    p.sf_h = m.d_patch_size.get();
    p.nsub = m.nsub;
    p.out = starttimes0;
    p.chain_bad = chain_bad;
    int nmax = 0;
    for (int s = 0; s < m.nsub; s++) nmax = std::max(nmax, m.ndip[s] * m.nstrike[s]);
    return launch_sweep(ctx, p, nmax);
}

}  // namespace beatamd
