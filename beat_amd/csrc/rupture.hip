// rupture.hip -- the arrays behind the FFI slip-distribution figure (plotting/ffi.py:338-398 fuzzy_rupture_fronts, :401-762
// fault_slip_distribution): contour lines of the start times of an ensemble of draws (what the reference gets from one
// matplotlib contour call per draw, :599-611) and the density grid of arbitrary polylines (its loop of draw_line_on_array
// over the contour lines, plotting/common.py:619-801).  The orders the kernels promise are stated at each kernel.
#include "devmath.hpp"
#include "kernels.hpp"
#include "raster.hpp"
#include "wave.hpp"

namespace beatamd {

// ---- min and max of the start times of every (draw, subfault): one wavefront each; a non-finite start time makes both NaN
__global__ void __launch_bounds__(64) k_rupture_minmax(int64_t ncells_total, const double *sts, int nsub, const int64_t *subs,
                                                       double *out)
{
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, e = w / nsub;
    const int sub = (int)(w % nsub);
    const int64_t *sb = subs + CT_SUB_FIELDS * sub;
    const int64_t n = sb[0] * sb[1];
    const double *z = sts + e * ncells_total + sb[2];
    double lo = __builtin_inf(), hi = -__builtin_inf();
    int bad = 0;
    for (int64_t k = lane; k < n; k += 64) {
        const double v = z[k];
        if (!is_finite(v)) bad = 1;
        lo = fmin(lo, v);
        hi = fmax(hi, v);
    }
    lo = wave_butterfly<OpFmin>(lo);
    hi = wave_butterfly<OpFmax>(hi);
    bad = wave_butterfly<OpMax>(bad);
    if (lane == 0) {
        out[2 * w] = bad ? __builtin_nan("") : lo;
        out[2 * w + 1] = bad ? __builtin_nan("") : hi;
    }
}

int launch_rupture_minmax(beatamd_ctx *ctx, int64_t E, int64_t ncells_total, const double *sts, int nsub, const int64_t *subs,
                          double *out)
{
    if (E * nsub == 0) return BEATAMD_OK;
    BA_CHECK(E * nsub < (int64_t)0x7fffffff, BEATAMD_EINVAL, "rupture_minmax: too many (draw, subfault) pairs in one call");
    hipLaunchKernelGGL(k_rupture_minmax, dim3((unsigned)(E * nsub)), dim3(64), 0, ctx->stream, ncells_total, sts, nsub, subs, out);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ---- contour lines by marching squares.  The cell (i, j) of a subfault of n_dip x n_strike nodes (row-major, i the dip
// index) has the corners 0 = a = (i, j), 1 = b = (i, j + 1), 2 = c = (i + 1, j + 1), 3 = d = (i + 1, j); its side k joins the
// corners k and k + 1 (mod 4).  A node is above iff z > level.  A segment is directed with the above side on its left in
// (j, i) index space: it ENTERS the cell through a side whose corner k is above and corner k + 1 is not, and LEAVES through
// one where corner k is not above and k + 1 is.  A saddle (a, c or b, d above) has two segments; with
// 0.25 (((za + zb) + zc) + zd) > level the segment entering through side s leaves through s + 1, else through s + 3 (mod 4);
// the segment with the lower entry side is slot 0.  The key of a segment is 2 (i (n_strike - 1) + j) + slot.
//
// Lines: the successor of a segment is the segment of the neighbouring cell that enters through the side it leaves
// through (an edge is crossed iff exactly one of its nodes is above, so both cells agree); no neighbour: the line ends
// there.  An open line starts at the segment without predecessor, a closed one at its segment with the smallest key; the
// lines of a level are ordered by the key of their first segment.  A line of n segments has n + 1 vertices: every segment's
// entry vertex, and the last segment's exit vertex (a closed line so repeats its first vertex, with the same bits: a vertex
// is a function of its edge alone).  On an edge with below-node p and above-node q
//     f = (z_q - level) / (z_q - z_p);  x = x_p f + x_q (1 - f);  y = y_p f + y_q (1 - f)        (never contracted)
//
// One wavefront <-> (draw, subfault, level); the subfault's start times and the link tables live in LDS.  lane <-> cell in
// rounds of 64 (links), lane <-> segment (every segment walks back to its line's start: rank = steps; a start walks forward
// for the length), then a scan over the keys numbers the lines and their first vertices.  No atomics: the output position
// of a vertex is a function of (draw, subfault, level, line, rank) alone.
struct CtArgs {
    int64_t ncells_total;
    int nsub;
    const double *sts;          // [E, ncells_total]
    const int64_t *subs;        // [nsub, CT_SUB_FIELDS] = (n_dip, n_strike, first cell, first x, first y)
    const double *x, *y;        // the centre coordinates of all subfaults, strike / dip
    const double *levels;       // [E, nsub, CT_LMAX]
    const int32_t *nlevels;     // [E, nsub]
    int32_t *counts;            // count pass: [E, nsub, CT_LMAX, 2] = (lines, vertices)
    const int64_t *line_base, *vert_base;   // fill pass: [E, nsub, CT_LMAX], the exclusive scans of the counts
    double *vertices;           // [V, 2]
    int64_t *line_offsets;      // [nlines + 1] (the last entry is the caller's)
    int64_t nlines, nverts;     // fill pass: the sizes of the two arrays; nothing is written beyond them
};

// the segments of a cell: n | entry0 << 2 | exit0 << 4 | entry1 << 6 | exit1 << 8
__device__ __forceinline__ int ct_cell(const double *z, int ns, int i, int j, double level)
{
#pragma clang fp contract(off)
    const double za = z[i * ns + j], zb = z[i * ns + j + 1], zc = z[(i + 1) * ns + j + 1], zd = z[(i + 1) * ns + j];
    const int mask = (za > level ? 1 : 0) | (zb > level ? 2 : 0) | (zc > level ? 4 : 0) | (zd > level ? 8 : 0);
    const int nxt = ((mask >> 1) | (mask << 3)) & 15;          // bit k: corner k + 1 is above
    const int ent = mask & ~nxt & 15, ext = ~mask & nxt & 15;
    if (!ent) return 0;
    const int e0 = __builtin_ctz(ent);
    if ((ent & (ent - 1)) == 0) return 1 | e0 << 2 | __builtin_ctz(ext) << 4;
    const int e1 = __builtin_ctz(ent & (ent - 1));
    const int turn = 0.25 * (((za + zb) + zc) + zd) > level ? 1 : 3;
    return 2 | e0 << 2 | ((e0 + turn) & 3) << 4 | e1 << 6 | ((e1 + turn) & 3) << 8;
}

// the segment on the other side of `side` of cell (i, j): the one that leaves (WANT_EXIT) / enters its cell through the
// shared edge; -1 where the grid ends
template <bool WANT_EXIT>
__device__ __forceinline__ int ct_neighbour(const double *z, int nd, int ns, int i, int j, int side, double level)
{
    const int ni = i + (side == 2) - (side == 0), nj = j + (side == 1) - (side == 3);
    if (ni < 0 || nj < 0 || ni >= nd - 1 || nj >= ns - 1) return -1;
    const int cc = ct_cell(z, ns, ni, nj, level), back = (side + 2) & 3;
    const int s0 = (cc >> (WANT_EXIT ? 4 : 2)) & 3;
    const int slot = ((cc & 3) == 2 && s0 != back) ? 1 : 0;
    return 2 * (ni * (ns - 1) + nj) + slot;
}

// the vertex on side `side` of cell (i, j)
__device__ __forceinline__ void ct_vertex(const double *z, const double *x, const double *y, int ns, int i, int j, int side,
                                          double level, double *vx, double *vy)
{
#pragma clang fp contract(off)
    const int k1 = (side + 1) & 3;
    const int i0 = i + (side >> 1), j0 = j + (((side + 1) >> 1) & 1), i1 = i + (k1 >> 1), j1 = j + (((k1 + 1) >> 1) & 1);
    const double z0 = z[i0 * ns + j0], z1 = z[i1 * ns + j1];
    const bool first_above = z0 > level;
    const int ip = first_above ? i1 : i0, jp = first_above ? j1 : j0, iq = first_above ? i0 : i1, jq = first_above ? j0 : j1;
    const double zp = first_above ? z1 : z0, zq = first_above ? z0 : z1;
    const double f = (zq - level) / (zq - zp);
    *vx = x[jp] * f + x[jq] * (1.0 - f);
    *vy = y[ip] * f + y[iq] * (1.0 - f);
}

template <bool FILL>
__device__ __forceinline__ void ct_body(const CtArgs &a, double *z)
{
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, es = w / CT_LMAX;
    const int l = (int)(w % CT_LMAX), sub = (int)(es % a.nsub);
    const int64_t e = es / a.nsub;
    const int64_t *sb = a.subs + CT_SUB_FIELDS * sub;
    const int nd = (int)sb[0], ns = (int)sb[1];
    if (l >= a.nlevels[es] || nd < 2 || ns < 2) {
        if (!FILL && lane == 0) a.counts[2 * w] = a.counts[2 * w + 1] = 0;
        return;
    }
    const int N = nd * ns, nc = (nd - 1) * (ns - 1), S = 2 * nc;
    int *pred = reinterpret_cast<int *>(z + N), *succ = pred + S, *start = succ + S, *rank = start + S, *lidx = rank + S,
        *loff = lidx + S;
    const double level = a.levels[w];
    const double *src = a.sts + e * a.ncells_total + sb[2];
    for (int k = lane; k < N; k += 64) z[k] = src[k];
    wave_lds_sync();
    // links; -2: the slot holds no segment
    for (int c = lane; c < nc; c += 64) {
        const int i = c / (ns - 1), j = c - i * (ns - 1);
        const int cc = ct_cell(z, ns, i, j, level), n = cc & 3;
        pred[2 * c] = n > 0 ? ct_neighbour<true>(z, nd, ns, i, j, (cc >> 2) & 3, level) : -2;
        succ[2 * c] = n > 0 ? ct_neighbour<false>(z, nd, ns, i, j, (cc >> 4) & 3, level) : -2;
        pred[2 * c + 1] = n > 1 ? ct_neighbour<true>(z, nd, ns, i, j, (cc >> 6) & 3, level) : -2;
        succ[2 * c + 1] = n > 1 ? ct_neighbour<false>(z, nd, ns, i, j, (cc >> 8) & 3, level) : -2;
    }
    wave_lds_sync();
    // every segment walks back to the start of its line (every walk ends after at most S steps whatever the tables hold)
    for (int s = lane; s < S; s += 64) {
        int st = -1, rk = 0, len = 0;
        if (pred[s] != -2) {
            int cur = s, steps = 0, mn = s, kmin = 0;
            st = s;
            for (; steps <= S;) {
                const int p = pred[cur];
                if (p < 0) { st = cur; rk = steps; break; }         // open: the segment without predecessor
                if (p == s) { st = mn; rk = kmin; break; }          // closed: the smallest key, kmin steps back
                cur = p;
                steps++;
                if (cur < mn) { mn = cur; kmin = steps; }
            }
            if (st == s) {                                          // a start: the segments of its line
                len = 1;
                for (cur = s; len <= S; len++) {
                    const int q = succ[cur];
                    if (q < 0 || q == s) break;
                    cur = q;
                }
            }
        }
        start[s] = st;
        rank[s] = rk;
        loff[s] = st == s ? len + 1 : 0;                            // (vertices of the line that starts here)
    }
    wave_lds_sync();
    // scan over the keys: the number of a start's line and of its first vertex within the level
    int nlines = 0, nverts = 0;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const int nv = s < S ? loff[s] : 0, fl = nv > 0 ? 1 : 0;
        int cl = fl, cv = nv;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int tl = __shfl_up(cl, d), tv = __shfl_up(cv, d);
            if (lane >= d) { cl += tl; cv += tv; }
        }
        if (s < S) { lidx[s] = nlines + cl - fl; loff[s] = nverts + cv - nv; }
        nlines += __shfl(cl, 63);
        nverts += __shfl(cv, 63);
    }
    if (!FILL) {
        if (lane == 0) { a.counts[2 * w] = nlines; a.counts[2 * w + 1] = nverts; }
        return;
    }
    wave_lds_sync();
    const int64_t lb = a.line_base[w], vb = a.vert_base[w];
    const double *x = a.x + sb[3], *y = a.y + sb[4];
    for (int s = lane; s < S; s += 64) {
        const int st = start[s];
        if (st < 0) continue;
        const int c = s >> 1, i = c / (ns - 1), j = c - i * (ns - 1);
        const int cc = ct_cell(z, ns, i, j, level), sh = (s & 1) ? 6 : 2;
        const int64_t at = vb + loff[st] + rank[s];
        double vx, vy;
        ct_vertex(z, x, y, ns, i, j, (cc >> sh) & 3, level, &vx, &vy);
        if (at < a.nverts) {
            a.vertices[2 * at] = vx;
            a.vertices[2 * at + 1] = vy;
        }
        const int q = succ[s];
        if ((q < 0 || q == st) && at + 1 < a.nverts) {
            ct_vertex(z, x, y, ns, i, j, (cc >> (sh + 2)) & 3, level, &vx, &vy);
            a.vertices[2 * at + 2] = vx;
            a.vertices[2 * at + 3] = vy;
        }
        if (st == s && lb + lidx[s] < a.nlines) a.line_offsets[lb + lidx[s]] = vb + loff[s];
    }
}

__global__ void __launch_bounds__(64) k_contour_count(CtArgs a)
{
    extern __shared__ double ct_lds[];
    ct_body<false>(a, ct_lds);
}

__global__ void __launch_bounds__(64) k_contour_fill(CtArgs a)
{
    extern __shared__ double ct_lds[];
    ct_body<true>(a, ct_lds);
}

int launch_contours(beatamd_ctx *ctx, int64_t E, int64_t ncells_total, const double *sts, int nsub, const int64_t *subs,
                    int64_t max_nodes, const double *x, const double *y, const double *levels, const int32_t *nlevels,
                    int32_t *counts, const int64_t *line_base, const int64_t *vert_base, int64_t nlines, int64_t nverts, double *vertices,
                    int64_t *line_offsets)
{
    if (E * nsub == 0) return BEATAMD_OK;
    BA_CHECK(max_nodes <= CT_MAX_NODES, BEATAMD_EINVAL, "contours: a subfault of %lld patches (at most %d: the start times and "
             "the link tables of a subfault live in LDS)", (long long)max_nodes, CT_MAX_NODES);
    BA_CHECK(E * nsub * CT_LMAX < (int64_t)0x7fffffff, BEATAMD_EINVAL, "contours: too many (draw, subfault, level) triples in one call");
    CtArgs a;
    a.ncells_total = ncells_total; a.nsub = nsub; a.sts = sts; a.subs = subs; a.x = x; a.y = y; a.levels = levels;
    a.nlevels = nlevels; a.counts = counts; a.line_base = line_base; a.vert_base = vert_base; a.vertices = vertices;
    a.line_offsets = line_offsets; a.nlines = nlines; a.nverts = nverts;
    const size_t lds = ct_lds_bytes(max_nodes);
    const auto kern = counts ? k_contour_count : k_contour_fill;
    if (lds > 64 * 1024) BA_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ScopedTimer tm(ctx, counts ? "contour_count" : "contour_fill");
    hipLaunchKernelGGL(kern, dim3((unsigned)(E * nsub * CT_LMAX)), dim3(64), lds, ctx->stream, a);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// ---- density grid of polylines (plotting/ffi.py:374-385: draw_line_on_array once per contour line).  Every selected
// polyline is drawn as its segments, anti-aliased, into an image of its own -- a pixel keeps the value of the
// highest-numbered segment that writes it -- and the image is added to the grid, polylines in the order given; coverage
// gets 1 per polyline wherever its image is positive.  The rasteriser is raster.hpp's, the one k_trace_density
// (summary.hip) draws with; what is here is where the segments come from: the vertices are arbitrary, so a workgroup
// cannot find its segments by bisection on a time axis.
struct PdArgs {
    int64_t nsel;
    const int64_t *sel, *line_offsets;   // sel [nsel]: the polylines to draw, in order (nullptr: 0 ... nsel - 1)
    const double *vertices;              // [V, 2] = (x, y)
    double xmin, xstep, ymin, ystep, linewidth;
    int ny, nx, strip, rows, pad;
    double *grid;                        // [ny, nx]
    int32_t *coverage;                   // [ny, nx] or nullptr
    int32_t *bbox;                       // [nsel, 4] = (first column, last column, first row, last row) of the cell indices
    int *status;
};

// one wavefront <-> a selected polyline: every vertex's cell indices are checked (rs_index_status; a vertex raises one word,
// not finite before out of the grid) and their bounding box is kept
__global__ void __launch_bounds__(256) k_polyline_check(PdArgs a)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t li = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (li >= a.nsel) return;
    const int64_t L = a.sel ? a.sel[li] : li;
    const int64_t v0 = a.line_offsets[L], n = a.line_offsets[L + 1] - v0;
    int bad = 0, cmin = 0x7fffffff, cmax = -0x7fffffff, rmin = 0x7fffffff, rmax = -0x7fffffff;
    if (!(a.xstep > 0.0) && n > 0) bad |= ST_LINE_NONFINITE;
    for (int64_t k = lane; k < n; k += 64) {
        const double c = rs_cell(a.vertices[2 * (v0 + k)], a.xmin, a.xstep);
        const double r = rs_cell(a.vertices[2 * (v0 + k) + 1], a.ymin, a.ystep);
        const int st = rs_index_status(c, a.nx - 1) | rs_index_status(r, a.ny - 1);
        if (st) bad |= st & ST_LINE_NONFINITE ? ST_LINE_NONFINITE : ST_LINE_OOB;
        else {
            cmin = min(cmin, (int)c); cmax = max(cmax, (int)c);
            rmin = min(rmin, (int)r); rmax = max(rmax, (int)r);
        }
    }
    if (bad) atomicOr(a.status, bad);
    cmin = wave_butterfly<OpMin>(cmin); cmax = wave_butterfly<OpMax>(cmax);
    rmin = wave_butterfly<OpMin>(rmin); rmax = wave_butterfly<OpMax>(rmax);
    if (lane == 0) {
        int32_t *bb = a.bbox + 4 * li;
        bb[0] = cmin; bb[1] = cmax; bb[2] = rmin; bb[3] = rmax;
    }
}

// The set-up (raster.hpp) of the RS_THREADS segments of the polyline v from seg0 on (the last is ihi) for the workgroup's
// tile; segment i joins the vertices i - 1 and i.  -> its pairs: the segments that can touch the tile are the only ones
// the passes see
__device__ __forceinline__ int pd_setup(const PdArgs &a, RsSetup &S, const double *v, int64_t seg0, int64_t ihi, int s0, int s1,
                                        int t0, int t1)
{
    const int64_t i = seg0 + threadIdx.x;
    const bool have = i <= ihi;
    int c0 = 0, r0 = 0, c1 = 0, r1 = 0;
    if (have) {
        c0 = (int)rs_cell(v[2 * (i - 1)], a.xmin, a.xstep);
        c1 = (int)rs_cell(v[2 * i], a.xmin, a.xstep);
        r0 = (int)rs_cell(v[2 * (i - 1) + 1], a.ymin, a.ystep);
        r1 = (int)rs_cell(v[2 * i + 1], a.ymin, a.ystep);
    }
    return rs_setup(S, have, c0, r0, c1, r1, a.linewidth, s0, s1, t0, t1);
}

// One workgroup <-> a tile of the grid; it walks the polylines in order, so every pixel's sum has the reference's order
// without atomics on doubles, and the tile is the workgroup's alone.  A polyline whose bounding box (k_polyline_check),
// widened by `pad` cells, misses the tile is passed over without a barrier.  The result does not depend on the tile's
// shape or on the chunking.
__global__ void __launch_bounds__(RS_THREADS) k_polyline_density(PdArgs a)
{
    extern __shared__ uint32_t pd_owner[];
    __shared__ RsSetup S;
    if (*(volatile int *)a.status & (ST_LINE_OOB | ST_LINE_NONFINITE)) return;   // (k_polyline_check, uniform)
    const int s0 = blockIdx.x * a.strip, s1 = min(s0 + a.strip, a.nx - 1);
    const int t0 = blockIdx.y * a.rows, t1 = min(t0 + a.rows, a.ny - 1);
    if (s0 >= s1 || t0 >= t1) return;
    for (int k = threadIdx.x; k < a.rows * a.strip; k += RS_THREADS) pd_owner[k] = 0u;
    __syncthreads();
    for (int64_t li = 0; li < a.nsel; li++) {
        const int32_t *bb = a.bbox + 4 * li;
        if (bb[1] + a.pad < s0 || bb[0] - a.pad >= s1 || bb[3] + a.pad < t0 || bb[2] - a.pad >= t1) continue;
        const int64_t L = a.sel ? a.sel[li] : li;
        const int64_t v0 = a.line_offsets[L], hi = a.line_offsets[L + 1] - v0 - 1;    // segments 1 ... hi
        if (hi < 1) continue;
        const double *v = a.vertices + 2 * v0;
        const bool single = hi <= RS_THREADS;
        int total = 0;
        for (int64_t seg0 = 1; seg0 <= hi; seg0 += RS_THREADS) {
            total = pd_setup(a, S, v, seg0, hi, s0, s1, t0, t1);
            rs_pass<0>(S, pd_owner, a.strip, a.grid, a.coverage, a.nx, seg0, total, s0, s1, t0, t1);
            __syncthreads();
        }
        for (int64_t seg0 = 1; seg0 <= hi; seg0 += RS_THREADS) {
            if (!single) total = pd_setup(a, S, v, seg0, hi, s0, s1, t0, t1);
            rs_pass<1>(S, pd_owner, a.strip, a.grid, a.coverage, a.nx, seg0, total, s0, s1, t0, t1);
            __syncthreads();
        }
    }
}

int launch_polyline_density(beatamd_ctx *ctx, int64_t nsel, const int64_t *sel, const int64_t *line_offsets,
                            const double *vertices, const double *extent, int64_t ny, int64_t nx, double linewidth, double *grid,
                            int32_t *coverage)
{
    BA_TRY(rs_check_args("polyline_density", ny, nx, linewidth));
    BA_CHECK(nsel >= 0 && (nsel + 3) / 4 < (int64_t)0x7fffffff, BEATAMD_EINVAL, "polyline_density: bad polyline count");
    if (nsel == 0) return BEATAMD_OK;
    PdArgs a;
    a.nsel = nsel; a.sel = sel; a.line_offsets = line_offsets; a.vertices = vertices; a.linewidth = linewidth;
    a.xmin = extent[0]; a.ymin = extent[2];
    a.xstep = (extent[1] - extent[0]) / (double)(nx - 1);
    a.ystep = (extent[3] - extent[2]) / (double)(ny - 1);
    a.ny = (int)ny; a.nx = (int)nx; a.grid = grid; a.coverage = coverage; a.status = ctx->d_status;
    BA_TRY(ctx->scratch(SL_PD_BOX, (size_t)4 * nsel, &a.bbox));
    a.pad = rs_pad(linewidth);
    // BEATAMD_PD_STRIP / BEATAMD_PD_ROWS: test knobs for the tile's shape, the result does not change
    const GfKnobs &kn = gf_knobs(ctx);
    a.strip = std::max(1, std::min(GfKnobs::get(kn.pd_strip, PD_STRIP), (int)nx));
    a.rows = std::max(1, std::min(GfKnobs::get(kn.pd_rows, PD_ROWS), (int)ny));
    a.rows = std::max(1, std::min(a.rows, PD_LDS_BYTES / (4 * a.strip)));
    const size_t lds = (size_t)a.rows * a.strip * sizeof(uint32_t);
    if (lds + sizeof(RsSetup) > 64 * 1024)
        BA_HIP(hipFuncSetAttribute((const void *)k_polyline_density, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ScopedTimer tm(ctx, "polyline_density");
    hipLaunchKernelGGL(k_polyline_check, dim3((unsigned)((nsel + 3) / 4)), dim3(256), 0, ctx->stream, a);
    BA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_polyline_density, dim3((unsigned)((nx - 1 + a.strip - 1) / a.strip), (unsigned)((ny - 1 + a.rows - 1) / a.rows)),
                       dim3(RS_THREADS), lds, ctx->stream, a);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
