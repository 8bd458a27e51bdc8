// metropolis.hpp -- the rules of a Metropolis step as device functions, one definition each: the proposal of a
// component with its prior-box test, the accept predicate, `like` of a likelihood row and the step-size table.  The
// step-by-step kernels (k_propose, k_accept, k_like_sum, k_like_assemble, k_tune_scaling) and the fused ones
// (k_draw_propose, k_hyper_chain) call these, so every path proposes, accepts and tunes bit for bit alike.  The draws
// are philox.hpp.
#pragma once
#include "kernels.hpp"
#include "philox.hpp"

#define LOG_2PI 1.8378770664093453  // log(2*pi), distributions.py:13

#ifdef __HIPCC__
namespace beatamd {

// metropolis.py:313-343: q = q0 + delta * scaling; prior_logp finite <=> lower <= q <= upper.  -> inside the box (a
// NaN is outside).  Outside the box the reference does not evaluate the forward model and the chain stays
// (metropolis.py:341-343, 383-385); the callers park such a chain on q0.
__device__ __forceinline__ bool propose_component(double q0, double delta, double sc, double lo, double up, double &q)
{
    const double d = delta * sc;
    q = q0 + d;
    return q >= lo && q <= up;   // the callers test !inside, i.e. !(q >= lo && q <= up): true of a NaN
}

// metropolis.py:344-385 + pymc metrop_select: accept iff isfinite(mr) and log u < mr, mr = beta (lp - l0)
__device__ __forceinline__ bool metropolis_accept(double beta, double lp, double l0, double log_u)
{
    const double mr = beta * (lp - l0);
    return isfinite(mr) && (log_u < mr);
}

// problems.py:227-247: like = sum over composites of (composite llk vector).sum(), one thread walking the row l
// (global or LDS) in order: per composite ascending, then over composites.  A chain flagged `bad` (its start times /
// durations left the library grid, where the reference raises IndexError) carries NaN, which metropolis_accept rejects.
__device__ __forceinline__ double like_serial(const double *l, const LikeGroups &grp, bool bad)
{
    double total = 0.0;
    int k = 0;
    for (int g = 0; g < grp.n; g++) {
        double s = 0.0;
        for (; k < grp.end[g]; k++) s += l[k];
        total += s;
    }
    if (bad) total = __builtin_nan("");
    return total;
}

// metropolis.py:294-306 with pymc's tune table (restated from its documentation):
//   acc < 0.001 x0.1 | < 0.05 x0.5 | < 0.2 x0.9 | > 0.95 x10 | > 0.75 x2 | > 0.5 x1.1
__device__ __forceinline__ double tune_factor(double acc)
{
    double f = 1.0;
    if (acc < 0.001) f = 0.1;
    else if (acc < 0.05) f = 0.5;
    else if (acc < 0.2) f = 0.9;
    else if (acc > 0.95) f = 10.0;
    else if (acc > 0.75) f = 2.0;
    else if (acc > 0.5) f = 1.1;
    return f;
}

}  // namespace beatamd
#endif
