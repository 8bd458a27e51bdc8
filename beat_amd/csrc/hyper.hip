// hyper.hip -- the hyper-parameter model (`beat sample --hypers`): the likelihood of the noise scalings h given each
// dataset's CACHED whitened misfit, and a whole Metropolis run on it in one launch.
//
// Reference arithmetic (hvasbath/beat):
//   hyper_normal          beat/models/distributions.py:176-222   dataset terms (through Composite.get_hyper_formula,
//                                                                 models/base.py:110-123)
//   _eval_prior           beat/models/laplacian.py:88-96, 156-170 one term per slip variable
//   built_hyper_model     beat/models/problems.py:261-297         like = sum over composites of the composite sums
//   Metropolis.astep      beat/sampler/metropolis.py:294-306, 313-385
//
// The forward model is gone from this chain: a step is a few hundred flops, so the step-by-step path (draw, propose,
// k_hyper_logp, accept, now and then tune) is bound by its launches.  The chains never talk to each other, hence
// k_hyper_chain runs ALL steps of a chain inside one kernel: one wavefront per chain, lanes over hyper-parameters and
// terms, the chain's state in LDS, no barrier between wavefronts after the tables are staged, no atomics but the final
// acceptance count.  Both paths call the same device functions, so they agree bit for bit: the draws
// (philox_univariate_pair, philox_log_u: philox.hpp), the proposal with its box test, the accept rule and the tuning
// table (propose_component, metropolis_accept, tune_factor: metropolis.hpp), the term formula and `like` (hyper_term,
// hyper_like below, shared with k_hyper_logp).
#include "kernels.hpp"
#include "metropolis.hpp"
#include "wave.hpp"

namespace beatamd {

// kind 0 (dataset, distributions.py:212-219; M = data.samples uncast, no M log 2pi):
//     -0.5 * (slog_pdet + (M * 2 * hp) + (1 / exp(hp * 2)) * llk)
// kind 1 (Laplacian, laplacian.py:92-96; slog = log-determinant of the operator, M = patches):
//     -0.5 * (-slog + (M * (LOG_2PI + 2 * hp)) + (1.0 / exp(hp * 2) * llk))
__device__ __forceinline__ double hyper_term(int kind, double M, double slog, double h, double llk)
{
#pragma clang fp contract(off)
    if (kind == 0) return (-0.5) * (slog + (M * 2 * h) + (1 / exp(h * 2)) * llk);
    return (-0.5) * (-slog + (M * (LOG_2PI + 2 * h)) + (1.0 / exp(h * 2) * llk));
}

// `like` of one chain by its wavefront (all 64 lanes call; every lane returns the same bits): per composite, lane l
// sums the terms l, l + 64, ... in ascending order, the 64 partial sums meet in a butterfly (xor 32, 16, ... 1), and the
// composite sums are added in composite order (problems.py:286-296).  The order depends on (nterm, group ends) only.
// (Not like_serial's order, on purpose: that one is a single thread walking the row.)
__device__ __forceinline__ double hyper_like(const double *terms, const LikeGroups &grp, int lane)
{
#pragma clang fp contract(off)
    double total = 0.0;
    int k0 = 0;
    for (int g = 0; g < grp.n; g++) {
        double s = 0.0;
        for (int k = k0 + lane; k < grp.end[g]; k += 64) s += terms[k];
        total += wave_butterfly<OpAdd>(s);
        k0 = grp.end[g];
    }
    return total;
}

struct HyperTables {
    int nterm, nh;
    const double *M, *slog;           // [nterm]
    const int32_t *kind, *hp_index;   // [nterm]
    LikeGroups grp;
};

constexpr int HY_WAVES = 4;   // chains per workgroup

// LL[c, :] = (terms, like) of H[c, :] given llks[c, :]; one wavefront per chain, the terms of a chain pass through LDS
__global__ void __launch_bounds__(64 * HY_WAVES) k_hyper_logp(HyperTables t, int64_t C, const double *H, const double *llks,
                                                            double *LL)
{
    extern __shared__ __attribute__((aligned(16))) double s_hy[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * HY_WAVES + wave;
    if (c >= C) return;
    double *terms = s_hy + (size_t)wave * t.nterm;
    const double *h = H + c * t.nh, *l = llks + c * t.nterm;
    double *out = LL + c * (t.nterm + 1);
    for (int k = lane; k < t.nterm; k += 64) {
        const double v = hyper_term(t.kind[k], t.M[k], t.slog[k], h[t.hp_index[k]], l[k]);
        terms[k] = v;
        out[k] = v;
    }
    wave_lds_fence_acqrel();
    const double like = hyper_like(terms, t.grp, lane);
    if (lane == 0) out[t.nterm] = like;
}

struct HyperChainArgs {
    HyperTables t;
    int64_t C;
    double *H, *LL, *scaling;       // [C, nh], [C, nterm + 1], [C]      in / out
    int32_t *acc_since;             // [C]                               in / out
    const double *llks;             // [C, nterm]
    const double *lower, *upper, *scales;   // [nh]
    int kind;                       // proposal family 0 / 1 / 2
    uint64_t seed, first_chain;
    uint32_t step0;
    int tune_interval, steps_until_tune;
    int64_t n_steps;
    int bt;                         // buffer_thinning
    double *trace;                  // [ndraws, C, nh + nterm + 1] or nullptr
    unsigned long long *n_acc;      // nullable
    int waves;                      // chains per workgroup
};

// LDS: the tables once per workgroup (M, slog [nterm]; lower, upper, scales [nh]; kind, hp_index [nterm]), then per
// wavefront its chain: h, hprop [nh]; cur, prop, llk [nterm]
__host__ __device__ inline size_t hyper_chain_lds(int nh, int nterm, int waves)
{
    return (size_t)nterm * 24 + (size_t)nh * 24 + (size_t)waves * ((size_t)nh * 16 + (size_t)nterm * 24);
}

__global__ void __launch_bounds__(64 * HY_WAVES) k_hyper_chain(HyperChainArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double s_hy[];
    const int nterm = a.t.nterm, nh = a.t.nh;
    double *sM = s_hy, *sslog = sM + nterm, *slo = sslog + nterm, *sup = slo + nh, *ssc = sup + nh;
    double *per = ssc + nh;
    int32_t *skind = (int32_t *)(per + (size_t)a.waves * (2 * nh + 3 * nterm)), *shp = skind + nterm;
    for (int k = threadIdx.x; k < nterm; k += blockDim.x) {
        sM[k] = a.t.M[k]; sslog[k] = a.t.slog[k]; skind[k] = a.t.kind[k]; shp[k] = a.t.hp_index[k];
    }
    for (int k = threadIdx.x; k < nh; k += blockDim.x) {
        slo[k] = a.lower[k]; sup[k] = a.upper[k]; ssc[k] = a.scales[k];
    }
    __syncthreads();   // the only workgroup barrier: from here on a wavefront is on its own
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * a.waves + wave;
    if (c >= a.C) return;
    double *h = per + (size_t)wave * (2 * nh + 3 * nterm), *hp = h + nh, *cur = hp + nh, *prop = cur + nterm,
           *llk = prop + nterm;
    const int64_t ld = nterm + 1;
    for (int k = lane; k < nh; k += 64) h[k] = a.H[c * nh + k];
    for (int k = lane; k < nterm; k += 64) {
        cur[k] = a.LL[c * ld + k];
        llk[k] = a.llks[c * nterm + k];
    }
    double lcur = a.LL[c * ld + nterm];
    double sc = a.scaling[c];
    int acc_since = a.acc_since[c], sut = a.steps_until_tune;
    unsigned long long nacc = 0;
    const uint32_t gc = (uint32_t)(a.first_chain + (uint64_t)c);
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const int npair = (nh + 1) / 2;
    const int64_t width = nh + nterm + 1;
    const int64_t first_rec = (a.n_steps - 1) % a.bt;
    wave_lds_fence_acqrel();

    for (int64_t s = 0; s < a.n_steps; s++) {
        // BatchedMetropolis._tune_if_due, ahead of the step's draws
        if (a.tune_interval > 0 && sut == 0) {
            sc = sc * tune_factor((double)acc_since / (double)a.tune_interval);
            acc_since = 0;
            sut = a.tune_interval;
        }
        const uint32_t step = a.step0 + (uint32_t)s;
        // k_philox_univariate + k_propose: delta = draw * scale, then propose_component
        bool ok = true;
        for (int j = lane; j < npair; j += 64) {
            double x, y;
            philox_univariate_pair(a.kind, (uint32_t)j, gc, step, k0, k1, x, y);
            const int k = 2 * j;
            if (!propose_component(h[k], x * ssc[k], sc, slo[k], sup[k], hp[k])) ok = false;
            if (k + 1 < nh && !propose_component(h[k + 1], y * ssc[k + 1], sc, slo[k + 1], sup[k + 1], hp[k + 1])) ok = false;
        }
        const double log_u = philox_log_u(gc, step, k0, k1);
        // outside the box: rejected without evaluation (metropolis.py:341-343, 383-385)
        if (__all(ok ? 1 : 0)) {
            wave_lds_fence_acqrel();
            for (int k = lane; k < nterm; k += 64) prop[k] = hyper_term(skind[k], sM[k], sslog[k], hp[shp[k]], llk[k]);
            wave_lds_fence_acqrel();
            const double lp = hyper_like(prop, a.t.grp, lane);
            if (metropolis_accept(1.0, lp, lcur, log_u)) {      // k_accept with beta = 1
                for (int j = lane; j < npair; j += 64) {      // (the lane that draws a pair owns its h)
                    h[2 * j] = hp[2 * j];
                    if (2 * j + 1 < nh) h[2 * j + 1] = hp[2 * j + 1];
                }
                for (int k = lane; k < nterm; k += 64) cur[k] = prop[k];
                lcur = lp;
                acc_since += 1;
                nacc += 1;
            }
        }
        sut -= 1;
        // the reference's buffer[-1::-buffer_thinning], reversed (beat/backend.py:113-115)
        if (a.trace && (a.n_steps - 1 - s) % a.bt == 0) {
            wave_lds_fence_acqrel();
            double *row = a.trace + (((s - first_rec) / a.bt) * a.C + c) * width;
            for (int k = lane; k < nh; k += 64) row[k] = h[k];
            for (int k = lane; k < nterm; k += 64) row[nh + k] = cur[k];
            if (lane == 0) row[nh + nterm] = lcur;
        }
    }
    wave_lds_fence_acqrel();
    for (int k = lane; k < nh; k += 64) a.H[c * nh + k] = h[k];
    for (int k = lane; k < nterm; k += 64) a.LL[c * ld + k] = cur[k];
    if (lane == 0) {
        a.LL[c * ld + nterm] = lcur;
        a.scaling[c] = sc;
        a.acc_since[c] = acc_since;
        if (a.n_acc && nacc) atomicAdd(a.n_acc, nacc);
    }
}

static HyperTables hyper_tables(const HyperModel &m)
{
    HyperTables t;
    t.nterm = (int)m.nterm; t.nh = (int)m.nh;
    t.M = m.M.get(); t.slog = m.slog.get(); t.kind = m.kind.get(); t.hp_index = m.hp_index.get();
    t.grp.n = m.ngroups;
    for (int g = 0; g < m.ngroups; g++) t.grp.end[g] = m.group_end[g];
    return t;
}

int launch_hyper_logp(beatamd_ctx *ctx, const HyperModel &m, int64_t C, const double *H, const double *llks, double *LL)
{
    if (C == 0) return BEATAMD_OK;
    const size_t lds = (size_t)HY_WAVES * m.nterm * sizeof(double);
    BA_CHECK(lds <= 64 * 1024, BEATAMD_EINVAL, "hyper_logp: %lld terms exceed the kernel's %d", (long long)m.nterm,
             64 * 1024 / 8 / HY_WAVES);
    ScopedTimer tm(ctx, "hyper");
    hipLaunchKernelGGL(k_hyper_logp, dim3((unsigned)((C + HY_WAVES - 1) / HY_WAVES)), dim3(64 * HY_WAVES), lds, ctx->stream,
                       hyper_tables(m), C, H, llks, LL);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

bool hyper_chain_applicable(int64_t nh, int64_t nterm) { return nh >= 1 && nh <= HYPER_CHAIN_MAX && nterm >= 1 && nterm <= HYPER_CHAIN_MAX; }

int launch_hyper_chain(beatamd_ctx *ctx, const HyperModel &m, const HyperChainCall &k)
{
    if (k.C == 0 || k.n_steps == 0) return BEATAMD_OK;
    HyperChainArgs a;
    a.t = hyper_tables(m);
    a.C = k.C; a.H = k.H; a.LL = k.LL; a.scaling = k.scaling; a.acc_since = k.acc_since; a.llks = k.llks;
    a.lower = k.lower; a.upper = k.upper; a.scales = k.scales; a.kind = k.kind; a.seed = k.seed;
    a.first_chain = k.first_chain; a.step0 = k.step0; a.tune_interval = k.tune_interval;
    a.steps_until_tune = k.steps_until_tune; a.n_steps = k.n_steps; a.bt = k.buffer_thinning; a.trace = k.trace;
    a.n_acc = (unsigned long long *)k.n_acc;
    // several chains per workgroup (a wavefront each: one per SIMD of a compute unit) while their state fits 64 KB of
    // LDS; a long model gets a workgroup per chain
    int waves = HY_WAVES;
    while (waves > 1 && hyper_chain_lds(a.t.nh, a.t.nterm, waves) > 64 * 1024) waves >>= 1;
    a.waves = waves;
    const size_t lds = hyper_chain_lds(a.t.nh, a.t.nterm, waves);
    if (lds > 64 * 1024)
        BA_HIP(hipFuncSetAttribute((const void *)k_hyper_chain, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ScopedTimer tm(ctx, "hyper");
    hipLaunchKernelGGL(k_hyper_chain, dim3((unsigned)((k.C + waves - 1) / waves)), dim3(64 * waves), lds, ctx->stream, a);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
