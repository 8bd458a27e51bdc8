// raster.hpp -- the anti-aliased line rasteriser of the two density kernels, k_trace_density (summary.hip) and
// k_polyline_density (rupture.hip), one definition each: plotting/common.py:619-801 draw_line_on_array / _weighted_line and
// utility.py:1556 positions2idxs.  The arithmetic is the reference's numpy arithmetic operation by operation (contraction
// off, correctly rounded sqrt): the grids are the reference's bit for bit.  The kernels differ in where their segments come
// from and in which of them they look at; that stays with them.
//
// A workgroup of RS_THREADS owns a tile of the grid, rows [t0, t1) x columns [s0, s1), and an owner map [t1 - t0, strip] in
// LDS (0 = nobody, segments count from 1).  It draws one line (a trace, a polyline) RS_THREADS segments at a time:
//   set-up  lane <-> segment: from the cell indices of its two end points the roles of rows and columns, slope, width,
//           intercept, and the range of x (the line's long axis) that lies inside the tile -> LDS; a segment that cannot
//           touch the tile gets no x at all.  An inclusive scan of the ranges' lengths numbers the (segment, x) pairs
//   pass    lane <-> (segment, x) pair, found by bisection in the scan -- a long steep segment is spread over the lanes
//           like many short ones; the lane walks the 2 th + 3 pixels across the line.  PASS 0: every pixel written gets
//           the segment number through an LDS atomic max; PASS 1: the same pixels again, and where the segment is the
//           owner its value is added to the grid, the coverage counted and the entry cleared: a pixel keeps the value of
//           the highest-numbered segment that writes it.
#pragma once
#include <cmath>

#include "ctx.hpp"
#include "devmath.hpp"

namespace beatamd {

constexpr int RS_THREADS = 256;
constexpr double RS_INDEX_MIN = -32768.0;   // below: the reference's int32 products overflow

// utility.py:1556: round((pos - min - cell / 2) / cell), half to even -- as a double
__device__ __forceinline__ double rs_cell(double pos, double lo, double step)
{
#pragma clang fp contract(off)
    return rint((pos - lo - step / 2.0) / step);
}

// the status word of one cell index on an axis of nmax + 1 cells: not finite -> ST_LINE_NONFINITE; above the grid or below
// RS_INDEX_MIN -> ST_LINE_OOB (check_line_in_grid's TypeError); else 0
__device__ __forceinline__ int rs_index_status(double q, int nmax)
{
    if (!is_finite(q)) return ST_LINE_NONFINITE;
    return q > (double)nmax || q < RS_INDEX_MIN ? ST_LINE_OOB : 0;
}

struct RsSetup {
    double slope[RS_THREADS], b[RS_THREADS], hw[RS_THREADS];
    int xlo[RS_THREADS], meta[RS_THREADS], pre[RS_THREADS];    // meta = th | transposed << 8; pre = scan of the lengths
    int wtot[RS_THREADS / 64];
};
static_assert(sizeof(RsSetup) <= 10 * 1024, "the launchers leave 10 KiB of LDS beside the owner map");

// The set-up of one chunk: the lane's segment joins the cells (c0, r0) and (c1, r1) (column, row); have: the lane has a
// segment at all.  Every thread of the workgroup calls it.  -> the chunk's number of (segment, x) pairs
__device__ __forceinline__ int rs_setup(RsSetup &S, bool have, int c0, int r0, int c1, int r1, double linewidth, int s0, int s1,
                                        int t0, int t1)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    int cnt = 0;
    if (have && (r0 != r1 || c0 != c1)) {                       // (else the reference's ValueError branch: nothing drawn)
        const bool tr = abs(c1 - c0) < abs(r1 - r0);            // steep: rows and columns change roles, limits included
        if (tr) { int s = r0; r0 = c0; c0 = s; s = r1; r1 = c1; c1 = s; }
        if (c0 > c1) { int s = r0; r0 = r1; r1 = s; s = c0; c0 = c1; c1 = s; }
        const double slope = (double)(r1 - r0) / (double)(c1 - c0);
        const double w = linewidth * sqrt(1.0 + fabs(slope)) / 2.0;
        const double b = (double)((int64_t)c1 * r0 - (int64_t)c0 * r1) / (double)(c1 - c0);
        const double hw = w / 2.0;
        const int th = (int)ceil(hw);
        // x runs along the long axis (columns, or rows when steep), y across it: both are cut to the tile, x here, y in
        // the pass
        const int xa = tr ? t0 : s0, xb = tr ? t1 : s1, ya = tr ? s0 : t0, yb = tr ? s1 : t1;
        const int xlo = max(c0, xa), xhi = min(c1, xb - 1);
        // Across the line the pixels lie within th + 2 of the end points' (th + 1 pixels and the centre's rounding): a
        // segment further from the tile than that gets no pairs.  This only saves work -- the pass clips y to [ya, yb)
        // itself, so such a segment would write no pixel -- and so may be applied to every segment, flat or steep
        const bool off = max(r0, r1) + th + 2 < ya || min(r0, r1) - th - 2 >= yb;
        if (xhi >= xlo && !off) cnt = xhi - xlo + 1;
        S.slope[tid] = slope; S.b[tid] = b; S.hw[tid] = hw; S.xlo[tid] = xlo; S.meta[tid] = th | (tr ? 256 : 0);
    }
    int v = cnt;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {   // a scan: open-coded (the reductions are wave.hpp's)
        const int n = __shfl_up(v, d);
        if (lane >= d) v += n;
    }
    if (lane == 63) S.wtot[wave] = v;
    __syncthreads();
    for (int k = 0; k < wave; k++) v += S.wtot[k];
    S.pre[tid] = v;
    __syncthreads();
    return S.pre[RS_THREADS - 1];
}

// One pass over the `total` pairs of the chunk that rs_setup left in S; its first segment has the number seg0.  grid
// [., nx] is addressed by the grid's own rows and columns; coverage (the same shape) may be nullptr
template <int PASS>
__device__ __forceinline__ void rs_pass(const RsSetup &S, uint32_t *owner, int strip, double *grid, int32_t *coverage, int nx,
                                        int64_t seg0, int total, int s0, int s1, int t0, int t1)
{
#pragma clang fp contract(off)
    for (int it = threadIdx.x; it < total; it += RS_THREADS) {
        int k = 0;                                              // the first segment whose scan exceeds `it`
#pragma unroll
        for (int s = RS_THREADS / 2; s > 0; s >>= 1)
            if (S.pre[k + s - 1] <= it) k += s;
        const int meta = S.meta[k], th = meta & 255;
        const bool tr = meta >> 8;
        const int x = S.xlo[k] + (it - (k ? S.pre[k - 1] : 0));
        const double slope = S.slope[k], b = S.b[k], hw = S.hw[k];
        const uint32_t seg = (uint32_t)(seg0 + k);
        const double ylo = tr ? (double)s0 : (double)t0, yhi = tr ? (double)s1 : (double)t1;
        const double yv = (double)x * slope + b;
        const double fl = floor(yv);
        for (int o = -th - 1; o <= th + 1; o++) {
            const double yy = fl + (double)o;
            const double up = yy + 1.0 + hw - yv, dn = -yy + 1.0 + hw + yv;
            double v = up < dn ? up : dn;
            v = v > 1.0 ? 1.0 : v;
            if (!(v > 0.0) || yy < ylo || !(yy < yhi)) continue;
            const int iy = (int)yy;
            const int row = tr ? x : iy, col = tr ? iy : x;
            uint32_t *own = owner + (row - t0) * strip + (col - s0);
            if (PASS == 0) {
                atomicMax(own, seg);
            } else if (*(volatile uint32_t *)own == seg) {
                const int64_t at = (int64_t)row * nx + col;
                grid[at] = grid[at] + v;
                if (coverage) coverage[at] = coverage[at] + 1;
                *own = 0u;
            }
        }
    }
}

// ---- host side, shared by the two launchers
// a line's half width is at most linewidth * sqrt(2) / 4, its pixels reach ceil(that) + 1 cells from the centre line; one
// more for the centre line's rounding
inline int rs_pad(double linewidth) { return (int)std::ceil(linewidth * 1.4142135623730951 / 4.0) + 2; }

// `who`: the entry's name, the prefix of its messages
inline int rs_check_args(const char *who, int64_t ny, int64_t nx, double linewidth)
{
    BA_CHECK(ny >= 2 && ny <= 4096 && nx >= 2 && nx <= 4096, BEATAMD_EINVAL, "%s: grid %lld x %lld (2 ... 4096 each)", who,
             (long long)ny, (long long)nx);
    BA_CHECK(linewidth > 0.0 && linewidth <= 64.0, BEATAMD_EINVAL, "%s: linewidth %g outside (0, 64]", who, linewidth);
    return BEATAMD_OK;
}

}  // namespace beatamd
