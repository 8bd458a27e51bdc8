// misfit.hpp -- the summation orders of the lane-per-chain misfits |W r|^2 as device functions, one definition each.  A
// chain's misfit has the same bits whichever kernel stacked it (batch size, group size, rank count, fused or not, patch
// ranges or not) because every path walks the trace in 64-sample tiles and calls these: k_gfstack_ws / _wsp / _dma / _dmaf
// (gfshared.hip), k_split_combine and k_sum_tiles (gfstack.hip), k_quadform_band1 (quadform.hip).  The generated runs
// program (gfruns_asm.inc, emulated by tools/gfcell_emu.py) states the same orders in assembly and is pinned against these
// paths by the tests.  The streaming kernel's wavefront tree, k_scalar_quad, k_quadform and k_quadform_banded are different
// orders by design.
//
// BIDIAGONAL operator (the reference's "exponential" noise structure, covariance.py:24-51; distributions.py:119-138 with a
// W of band 1; r = data - synthetics, seismic.py:1332) -- the CANONICAL order:
//     quad = 0;  for tile k = 0, 1, ...:   quad += q_k;   if (k is not the last tile) quad = fma(yb_k, yb_k, quad)
//     q_k  = sum over the tile's samples i but its last, ascending (fma(y_i, y_i, q)), + the trace's very last sample
//     y_i  = fma(W[i,i+1], r_{i+1}, fma(W[i,i], r_i, 0));  yb_k = y of the tile's last sample (its neighbour = next tile)
// SCALAR weight (W = w I):
//     quad = 0;  for tile k = 0, 1, ...:   quad += q_k;     q_k = sum over the tile's samples ascending (fma(t_i, t_i, q)),
//     t_i  = w (data_i - synthetics_i)
#pragma once

#ifdef __HIPCC__
namespace beatamd {

// (guard nullable) a guarded launch works only when (*guard != 0) == (want != 0): the two producers of a misfit, the runs
// kernel and its stand-in, each bring their own sums
__device__ __forceinline__ bool guard_skips(const int *guard, int want) { return guard && (*guard != 0) != (want != 0); }

// y of a sample with a neighbour, and of the trace's last sample (W[i,i+1] = 0 there: one product)
__device__ __forceinline__ double band1_y(double w0, double w1, double ri, double rn)
{
    double y = fma(w0, ri, 0.0);
    y = fma(w1, rn, y);
    return y;
}
__device__ __forceinline__ double band1_y(double w0, double ri) { return fma(w0, ri, 0.0); }

// sample i of a tile that has its neighbour at hand: q = fma(y_i, y_i, q), and the neighbour becomes r_i
template <class Res, class Band>
__device__ __forceinline__ void band1_step(const Res &r, const Band &w, int i, double &ri, double &q)
{
    const double rn = r(i + 1);
    const double y = band1_y(w(i, 0), w(i, 1), ri, rn);
    q = fma(y, y, q);
    ri = rn;
}

struct Band1Tile {
    double q;        // q_k
    double r_last;   // residual of the tile's last valid sample (the boundary term's r_i)
};

// q_k of a tile of nvalid (1 .. NT) samples, NT = the samples of a whole tile; r(i) = residual of the tile's sample i,
// w(i, 0 / 1) = W[i,i] / W[i,i+1] of it; trace_end: the tile's last valid sample is the trace's last.  How the samples are
// walked is the caller's generated code, the arithmetic and its order are the same: REGS8 = fully unrolled and predicated
// in groups of eight samples (accessors that index registers), else a loop over nvalid samples.  (k_quadform_band1 walks
// its tiles in loops of its own with band1_y: see there.)
template <bool REGS8, int NT, class Res, class Band>
__device__ __forceinline__ Band1Tile band1_tile(const Res &r, const Band &w, int nvalid, bool trace_end)
{
    double q = 0.0, ri = r(0);
    if constexpr (REGS8) {
#pragma unroll
        for (int i0 = 0; i0 < NT; i0 += 8) {
#pragma unroll
            for (int i = i0; i < i0 + 8; i++) {
                if (i + 1 < nvalid) {
                    band1_step(r, w, i, ri, q);
                } else if (i + 1 == nvalid && trace_end) {
                    const double y = band1_y(w(i, 0), ri);
                    q = fma(y, y, q);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        for (int i = 0; i + 1 < nvalid; i++) band1_step(r, w, i, ri, q);
        if (trace_end) {
            const double y = band1_y(w(nvalid - 1, 0), ri);
            q = fma(y, y, q);
        }
    }
    return {q, ri};
}

// the join over tiles, ascending: quad += q_k (both orders), and behind every tile but the trace's last its boundary term
// yb_k = band1_y(W of the tile's last sample, its residual, the next tile's first residual): in one call, or
// (k_quadform_band1, whose tile threads work yb_k out) in two
__device__ __forceinline__ double tile_join(double s, double q_k) { return s + q_k; }
__device__ __forceinline__ double band1_boundary(double s, double yb) { return fma(yb, yb, s); }
__device__ __forceinline__ double band1_join(double s, double q_k, bool has_boundary, double w0, double w1, double r_last,
                                             double r_next_first)
{
    s = tile_join(s, q_k);
    if (has_boundary) s = band1_boundary(s, band1_y(w0, w1, r_last, r_next_first));
    return s;
}

// scalar weight: t_i (seismic.py:1332), and q_k of a tile of nvalid (<= NT) samples; t(i) = t of the tile's sample i
__device__ __forceinline__ double scalar_t(double w, double data, double syn) { return w * (data - syn); }
template <bool REGS8, int NT, class T>
__device__ __forceinline__ double scalar_tile(const T &t, int nvalid)
{
    double q = 0.0;
    if constexpr (REGS8) {
#pragma unroll
        for (int i0 = 0; i0 < NT; i0 += 8) {
#pragma unroll
            for (int i = i0; i < i0 + 8; i++)
                if (i < nvalid) {
                    const double tt = t(i);
                    q = fma(tt, tt, q);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        for (int i = 0; i < nvalid; i++) {
            const double tt = t(i);
            q = fma(tt, tt, q);
        }
    }
    return q;
}

}  // namespace beatamd
#endif
