// polarity.hip -- first-motion polarity likelihood of a point-source moment tensor, batched over chains: the device
// counterpart of PolarityComposite.get_formula (beat/models/polarity.py:104-134).
//
// Per chain, from its parameter row q (PolSource: slot k = q[off[k]], or fix[k] where off[k] < 0):
//   moment tensor by source kind
//     POL_MTQT  (w, v, kappa, sigma, h), MTQTSource at rho = 1 (beat/sources.py:454-536, Tape & Tape 2015):
//         gamma = (1/3) asin(3 v) ;  beta = interp(3 pi / 8 - w, U_MAPPING, BETA_MAPPING) ;  theta = acos(h)
//         lambda = (1/sqrt 6) [[sqrt 3, -1, sqrt 2], [0, 2, sqrt 2], [-sqrt 3, -1, sqrt 2]] (sb cg, sb sg, cb)
//         U = Rz(-kappa) Rx(theta) Rz(sigma) Ry(-pi/4) ;  m_nwu = U diag(lambda) U^T ;  m9 = Rx(pi) m_nwu Rx(pi)^T
//       (utility.get_rotation_matrix's signs; U is orthogonal, the transpose is its inverse; Rx(pi) is taken as the
//       exact diag(1, -1, -1), Ry(-pi/4) with r = sqrt(1/2)).  The two 1000-point tables are data of the caller
//       (numpy builds them at set-up); pol_interp restates numpy.interp: its search, its exact-node and end cases and
//       its arithmetic slope * (x - xp[j]) + fp[j], without contraction -- equal bits, so the steep ends of the table
//       (slope ~ 2.5e10) cannot amplify a difference.
//     POL_MT    (mnn, mee, mdd, mne, mnd, med) as they are
//     POL_DC    (strike, dip, rake) [deg]: Aki & Richards (1980) box 4.4, north-east-down
//   then m9 /= sqrt(sum m9^2) / sqrt 2, the sum over all nine entries (heart.py:4086-4087; an all-zero tensor gives
//   NaN, which reaches `like` as in the reference), m6 = (mnn, mee, mdd, mne, mnd, med);
//   amplitudes  a[s] = ((((rw[0,s] m6[0] + rw[1,s] m6[1]) + rw[2,s] m6[2]) + rw[3,s] m6[3]) + rw[4,s] m6[4]) + rw[5,s] m6[5]
//   (heart.py:4088) with the station propagation coefficients rw [6, NT] of all maps side by side;
//   likelihood  p = g + (1 - 2 g) (0.5 + 0.5 erf((a / sigma) / sqrt 2)) ;
//               llk[s] = ((1 + o) / 2) log p + ((1 - o) / 2) log(1 - p)          (distributions.py:143-173)
//   sigma the hyper-parameter of the station's map AS IT IS (not exp), o the observed polarity.
//
// Layout: one wavefront per chain, four chains per workgroup.  Every lane forms the chain's tensor itself (the same
// instructions for 64 lanes as for one: nothing to broadcast, no LDS, no barrier), then the lanes stride over the
// stations.  A chain's numbers depend on its own row alone: how chains are batched changes no bit.  The work is a dozen
// transcendental calls per chain plus erf and two logarithms per station -- FP64 VALU bound, a few microseconds.
#include "kernels.hpp"
#include "mechanism.hpp"

namespace beatamd {

// numpy.interp (compiled arr_interp + binary_search_with_guess), one x
__device__ __forceinline__ double pol_interp(double x, const double *xp, const double *fp, int n)
{
#pragma clang fp contract(off)
    if (x != x) return x;
    if (x < xp[0]) return fp[0];
    if (x > xp[n - 1]) return fp[n - 1];
    int lo = 0, hi = n;   // xp[lo] <= x and (hi == n or x < xp[hi])
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (x >= xp[mid]) lo = mid;
        else hi = mid;
    }
    const int j = lo;
    if (j == n - 1 || xp[j] == x) return fp[j];
    const double slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
    double r = slope * (x - xp[j]) + fp[j];
    if (r != r) {
        r = slope * (x - xp[j + 1]) + fp[j + 1];
        if (r != r && fp[j] == fp[j + 1]) r = fp[j];
    }
    return r;
}

__device__ __forceinline__ double pol_w_to_beta(double w, const double *utab, const double *btab, int n)
{
#pragma clang fp contract(off)
    const double pi = 3.14159265358979323846;
    return pol_interp(3.0 * pi / 8.0 - w, utab, btab, n);
}

// the six independent entries BEFORE the normalisation
__device__ __forceinline__ void pol_mtqt(double w, double v, double kappa, double sigma, double h, const double *utab,
                                         const double *btab, int n, double *m)
{
#pragma clang fp contract(off)
    const double SQRT2 = 1.4142135623730951, SQRT3 = 1.7320508075688772, SQRT6 = 2.449489742783178;
    const double r = 0.7071067811865476;
    const double gamma = (1.0 / 3.0) * asin(3.0 * v);
    const double beta = pol_w_to_beta(w, utab, btab, n);
    const double theta = acos(h);
    const double sb = sin(beta), cb = cos(beta), sg = sin(gamma), cg = cos(gamma);
    const double v0 = sb * cg, v1 = sb * sg, v2 = cb;
    const double f = 1.0 / SQRT6;
    const double lam[3] = {f * ((SQRT3 * v0 - v1) + SQRT2 * v2), f * (2.0 * v1 + SQRT2 * v2),
                           f * ((-SQRT3 * v0 - v1) + SQRT2 * v2)};
    const double ck = cos(kappa), sk = sin(kappa), ct = cos(theta), st = sin(theta), cs = cos(sigma), ss = sin(sigma);
    // A = Rz(-kappa) Rx(theta)
    const double A[3][3] = {{ck, sk * ct, -(sk * st)}, {-sk, ck * ct, -(ck * st)}, {0.0, st, ct}};
    double U[3][3];
    for (int i = 0; i < 3; i++) {
        const double V0 = A[i][0] * cs + A[i][1] * ss, V1 = A[i][1] * cs - A[i][0] * ss, V2 = A[i][2];   // . Rz(sigma)
        U[i][0] = V0 * r + V2 * r;                                                                        // . Ry(-pi/4)
        U[i][1] = V1;
        U[i][2] = V2 * r - V0 * r;
    }
#define POL_M(i, j) ((U[i][0] * lam[0]) * U[j][0] + (U[i][1] * lam[1]) * U[j][1]) + (U[i][2] * lam[2]) * U[j][2]
    m[0] = POL_M(0, 0);
    m[1] = POL_M(1, 1);
    m[2] = POL_M(2, 2);
    m[3] = -(POL_M(0, 1));   // Rx(pi) = diag(1, -1, -1): north-west-up -> north-east-down
    m[4] = -(POL_M(0, 2));
    m[5] = POL_M(1, 2);
#undef POL_M
}

// the unit double couple of (strike, dip, rake) [deg]: mechanism.hpp states it once (k_mt_decompose reads it too)
__device__ __forceinline__ void pol_dc(double strike, double dip, double rake, double *m) { mech_dc_m6(strike, dip, rake, m); }

__device__ __forceinline__ void pol_m6(const PolSource &s, const double *Qc, const double *utab, const double *btab, int ntab,
                                       double *m)
{
#pragma clang fp contract(off)
    double p[6];
    const int nv = s.kind == POL_MTQT ? 5 : (s.kind == POL_MT ? 6 : 3);
    for (int k = 0; k < 6; k++) p[k] = k < nv ? (s.off[k] < 0 ? s.fix[k] : Qc[s.off[k]]) : 0.0;
    if (s.kind == POL_MTQT) pol_mtqt(p[0], p[1], p[2], p[3], p[4], utab, btab, ntab, m);
    else if (s.kind == POL_DC) pol_dc(p[0], p[1], p[2], m);
    else
        for (int k = 0; k < 6; k++) m[k] = p[k];
    // heart.py:4086-4087
    const double ssq = ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) + 2.0 * ((m[3] * m[3] + m[4] * m[4]) + m[5] * m[5]);
    const double scale = sqrt(ssq) / 1.4142135623730951;
    for (int k = 0; k < 6; k++) m[k] = m[k] / scale;
}

__device__ __forceinline__ double pol_amplitude(const double *rw, int64_t NT, int64_t s, const double *m)
{
#pragma clang fp contract(off)
    return ((((rw[s] * m[0] + rw[NT + s] * m[1]) + rw[2 * NT + s] * m[2]) + rw[3 * NT + s] * m[3]) + rw[4 * NT + s] * m[4]) +
           rw[5 * NT + s] * m[5];
}

// mode POL_OUT_LLK: out[c*ld + s] = llk of station s; POL_OUT_AMP: the amplitudes; POL_OUT_M6: out[c*ld + k] = m6[k].
// Chains with active[c] == 0 are skipped: their rows are not written
__global__ void __launch_bounds__(256) k_polarity(PolArgs a)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= a.C) return;
    if (a.active && a.active[c] == 0) return;
    const double *Qc = a.Q + c * a.nparams;
    double m[6];
    pol_m6(a.src, Qc, a.utab, a.btab, a.ntab, m);
    double *o = a.out + c * a.ld;
    if (a.mode == POL_OUT_M6) {
        if (lane < 6) o[lane] = m[lane];
        return;
    }
    int map = 0;
    for (int64_t s = lane; s < a.NT; s += 64) {
        const double amp = pol_amplitude(a.rw, a.NT, s, m);
        if (a.mode == POL_OUT_AMP) {
            o[s] = amp;
            continue;
        }
        while (map < a.nmap - 1 && s >= a.map_end[map]) map++;
        const double sigma = a.hp_off[map] < 0 ? a.hp_fix[map] : Qc[a.hp_off[map]];
        const double cn = 0.5 + 0.5 * erf((amp / sigma) / 1.4142135623730951);
        const double p = a.gamma + (1.0 - 2.0 * a.gamma) * cn;
        const double ob = a.obs[s];
        o[s] = ((1.0 + ob) / 2.0) * log(p) + ((1.0 - ob) / 2.0) * log(1.0 - p);
    }
}

int launch_polarity(beatamd_ctx *ctx, const PolArgs &a)
{
    if (a.C == 0) return BEATAMD_OK;
    const int64_t nb = (a.C + 3) / 4;
    BA_CHECK(nb < (int64_t)0x7fffffff, BEATAMD_EINVAL, "polarity: batch too large");
    BA_CHECK(a.src.kind != POL_MTQT || (a.ntab >= 2 && a.utab && a.btab), BEATAMD_EINVAL, "polarity: the mtqt source needs its tables");
    ScopedTimer tm(ctx, "polarity");
    hipLaunchKernelGGL(k_polarity, dim3((unsigned)nb), dim3(256), 0, ctx->stream, a);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

// sources.w_to_beta for n values: the device function the model's kernel calls
__global__ void __launch_bounds__(256) k_w_to_beta(int64_t n, const double *w, const double *utab, const double *btab, int ntab,
                                                  double *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = pol_w_to_beta(w[i], utab, btab, ntab);
}

int launch_w_to_beta(beatamd_ctx *ctx, int64_t n, const double *w, const double *utab, const double *btab, int ntab, double *out)
{
    if (n == 0) return BEATAMD_OK;
    const int64_t nb = (n + 255) / 256;
    BA_CHECK(nb < (int64_t)0x7fffffff && ntab >= 2, BEATAMD_EINVAL, "w_to_beta: bad size");
    hipLaunchKernelGGL(k_w_to_beta, dim3((unsigned)nb), dim3(256), 0, ctx->stream, n, w, utab, btab, ntab, out);
    BA_HIP(hipGetLastError());
    return BEATAMD_OK;
}

}  // namespace beatamd
