// okada.hpp -- the half-space source arithmetic shared by geometry.hip (line-of-sight synthetics of chains of
// sources) and geolib.hip (the geodetic Green's-function library of unit-slip patches): the per-source constants
// (source_const) and the surface displacement of one source at one point (source_disp).  Rectangular dislocation
// after Okada (1985), eqs 25-30, and the Mogi point source.  Stated once: both translation units compile this text.
#pragma once
#include "kernels.hpp"

// multiply-adds may contract here (the Makefile turns contraction off for the kernels that keep the
// reference's operation order; this arithmetic is pinned by tolerance to Okada's published values)
#pragma clang fp contract(fast)

namespace beatamd {

constexpr double GEOM_VERTICAL_COS = 1e-7;  // |cos(dip)| up to which I1..I5 take the vertical expressions (source_disp)
constexpr int GEO_NP = 10;  // east_shift north_shift depth strike dip rake length width slip opening

struct GeomSrcArgs {
    int nsrc;
    const int32_t *kind;     // [nsrc] 0 rectangular, 1 mogi
    const int64_t *poff;     // [nsrc*GEO_NP] offset in q, or -1 -> fixed value
    const double *pfix;      // [nsrc*GEO_NP]
    const double *Q;
    int64_t nparams, C, Nobs;
    const double *east, *north, *los;  // [Nobs], [Nobs], [Nobs,3] (Sn, Se, Su)
    double nu;
    double *mu;  // [C, Nobs] line-of-sight synthetics
    // with res: the weighted residual (data - mu) * odw is stored instead of mu
    const double *data, *odw;
    double *res;
    // k_geom_los<.., CORR = true>: the correction terms of the datasets, subtracted from res (unread otherwise)
    GeoCorr corr;
};

struct Vec3 { double x, y, z; };

// Okada (1985) eqs (25)-(30).  The displacement is Chinnery's sum f(x,p) - f(x,p-W) - f(x-L,p) +
// f(x-L,p-W) of a corner term f(xi, eta) that is LINEAR in ln(R+eta) and ln(R+d~) with coefficients
// that depend on the source only.  This kernel is bound by the fp64 VALU (an f64 log / atan / division
// is ~100 / ~100 / ~30 instructions), so the corner terms are accumulated with their signs in a form
// that needs per observation point
//     2 logarithms   ln[(R0+eta0)(R3+eta3) / ((R1+eta1)(R2+eta2))]  and the same for R+d~   (not 8)
//     1 division per corner: 1/R, 1/(R+eta), 1/(R+d~), 1/(R+xi) and the denominator of the I5 arc
//       tangent come out of ONE reciprocal of their product (not 6 divisions)
//     2 arc tangents and 2 square roots per corner (as written in the paper).
// Near a vertical dip I1 and I3 of the paper are differences of terms ~ 1/cos^2(dip): written as they stand they round
// like eps/cos^2(dip) (2e-11 slip at 89.9 deg, 2e-5 slip at 89.9999 deg).  Two identities take one power off:
//   * ln(R+d~) - sin ln(R+eta) = ln[(R+d~)/(R+eta)] + (1 - sin) ln(R+eta) with 1 - sin = cos t, t = cos/(1 + sin),
//     and (R+d~)/(R+eta) = 1 + x, x = -cos (eta t + q)/(R+eta): the Chinnery product of the (1 + x) is kept as its
//     distance from 1 (dp, dm below) and goes through log1p, so the second logarithm is O(cos) to full relative
//     precision and the term ~ sin/cos^2 ln(R+eta) is gone;
//   * atan(N/D) = sgn(N) sgn(D) pi/2 - atan(D/N) for the I5 arc tangent, D = xi (R+X) cos: the multiples of pi/2 are
//     counted exactly (they cancel in the Chinnery sum wherever N keeps its sign, as it does near vertical), the rest
//     is O(cos).
// What remains rounds like eps/|cos(dip)|; tests/test_gpu_geometry_mp.py holds it to multi-precision values.
struct CornerSum {
    // signed sums of the logarithm-free parts
    double ssx, ssy, ssz, dsx, dsy, dsz, tfx, tfy, tfz;
    // general dip: sums of -xi/(R+d~), of atan(D/N) and of sgn(N) sgn(D) ; vertical: I1, I5 themselves
    double i1, i5, k5, t3, i4r;
    // numerator / denominator of the argument of ln(R+eta); product - 1 of the (R+d~)/(R+eta) of the corners that
    // count positive / negative
    double re_n, re_d, dp, dm;
};

__device__ __forceinline__ void okada_corner(bool PLUS, double xi, double eta, double q, double rq, double sd,
                                             double cd, double rcd, double th /* cd / (1 + sd) */, bool vertical,
                                             double a /* mu/(lambda+mu) */, CornerSum &o)
{
    const double R = sqrt(xi * xi + eta * eta + q * q);
    const double yt = eta * cd + q * sd;
    const double dt = eta * sd - q * cd;
    const double X = sqrt(xi * xi + q * q);
    const double Re = R + eta, Rd = R + dt, Rx = R + xi;
    const bool xi0 = fabs(xi) < 1e-12;
    // the I5 arc tangent is atan(N5 / D5): evaluated as sgn pi/2 - atan(D5 / N5)
    const double N5 = eta * (X + q * cd) + X * (R + X) * sd, D5 = xi * (R + X) * cd;
    const bool no5 = xi0 || vertical || N5 == 0.0;
    const double den5 = no5 ? 1.0 : N5;
    // five reciprocals from one division
    const double p1 = R * Re, p2 = p1 * Rd, p3 = p2 * Rx, p4 = p3 * den5;
    const double inv = 1.0 / p4;
    const double rden5 = inv * p3;
    const double i3 = inv * den5;          // 1 / (R Re Rd Rx)
    const double rRx = i3 * p2;
    const double i2 = i3 * Rx;             // 1 / (R Re Rd)
    const double rRd = i2 * p1;
    const double i1_ = i2 * Rd;            // 1 / (R Re)
    const double rRe = i1_ * R;
    const double rR = i1_ * Re;
    double I1, I5, K5 = 0.0, t3, i4r;
    if (!vertical) {
        I5 = no5 ? 0.0 : atan(D5 * rden5);
        K5 = no5 ? 0.0 : ((N5 > 0.0) == (D5 > 0.0) ? 1.0 : -1.0);
        t3 = yt * rcd * rRd;
        i4r = 0.0;
        I1 = -xi * rRd;
    } else {
        I5 = -a * xi * sd * rRd;
        i4r = -a * q * rRd;
        t3 = eta * rRd + yt * q * (rRd * rRd);
        I1 = -a / 2.0 * xi * q * (rRd * rRd);
    }
    const double at = (fabs(q) < 1e-12) ? 0.0 : atan(xi * eta * rR * rq);
    const double qRe = q * i1_;            // q / (R (R + eta))
    const double qRx = q * rR * rRx;       // q / (R (R + xi))
    const double w = xi * qRe - at;
    const double sg = PLUS ? 1.0 : -1.0;
#define ACC(F, V) o.F = fma(sg, (V), o.F)
    ACC(ssx, xi * qRe + at);
    ACC(ssy, yt * qRe + q * cd * rRe);
    ACC(ssz, dt * qRe + q * sd * rRe);
    ACC(dsx, q * rR);
    ACC(dsy, yt * qRx + cd * at);
    ACC(dsz, dt * qRx + sd * at);
    ACC(tfx, q * qRe);
    ACC(tfy, -dt * qRx - sd * w);
    ACC(tfz, yt * qRx + cd * w);
    ACC(i1, I1);
    ACC(i5, I5);
    ACC(k5, K5);
    ACC(t3, t3);
    ACC(i4r, i4r);
#undef ACC
    o.re_n *= PLUS ? Re : 1.0;
    o.re_d *= PLUS ? 1.0 : Re;
    // (1 + dp) (1 + x) - 1
    const double x = -cd * (eta * th + q) * rRe;
    const double xp = PLUS ? x : 0.0, xm = PLUS ? 0.0 : x;
    o.dp = fma(o.dp, xp, o.dp + xp);
    o.dm = fma(o.dm, xm, o.dm + xm);
}

__device__ __forceinline__ double src_param(const GeomSrcArgs &a, const double *q, int s, int k)
{
    const int64_t o = a.poff[s * GEO_NP + k];
    return o >= 0 ? q[o] : a.pfix[s * GEO_NP + k];
}

// what one source of one chain contributes to every observation point: computed once per (chain,
// source) -- six sin/cos and the slip decomposition -- and kept in LDS by k_geom_los
struct SrcConst {
    double oe, on;        // rectangular: Okada origin (east, north) [km] ; Mogi: source position
    double ex, nx;        // along-strike unit vector (east, north)
    double sd, cd, rcd;   // sin / cos / 1/cos of the dip
    double th;            // cos / (1 + sin) of the dip
    double dbot, L, W;    // depth of the lower edge, length, width [km] ; Mogi: depth in dbot
    double U1, U2, U3;    // strike-slip, dip-slip, tensile components ; Mogi: volume change in U1
    int kind;
};

__device__ __forceinline__ void source_const(const GeomSrcArgs &a, const double *q, int s, SrcConst &k)
{
    const double D2R = 0.017453292519943295;
    const double es = src_param(a, q, s, 0), ns = src_param(a, q, s, 1);
    const double depth = src_param(a, q, s, 2);
    k.kind = a.kind[s];
    if (k.kind == 1) {
        k.oe = es; k.on = ns; k.dbot = depth; k.U1 = src_param(a, q, s, 8);
        return;
    }
    const double strike = src_param(a, q, s, 3) * D2R, dip = src_param(a, q, s, 4) * D2R;
    const double rake = src_param(a, q, s, 5) * D2R;
    k.L = src_param(a, q, s, 6);
    k.W = src_param(a, q, s, 7);
    const double slip = src_param(a, q, s, 8), f = src_param(a, q, s, 9);
    k.sd = sin(dip);
    k.cd = cos(dip);
    k.rcd = 1.0 / k.cd;
    k.th = k.cd / (1.0 + k.sd);
    k.ex = sin(strike);
    k.nx = cos(strike);
    const double ey = k.nx, ny = -k.ex;                 // horizontal down-dip direction
    k.dbot = depth + k.W * k.sd;
    k.oe = es - 0.5 * k.L * k.ex + k.W * k.cd * ey;
    k.on = ns - 0.5 * k.L * k.nx + k.W * k.cd * ny;
    const double shear = slip * (1.0 - fabs(f));
    k.U1 = shear * cos(rake);
    k.U2 = shear * sin(rake);
    k.U3 = slip * f;
}

// displacement (east, north, up) [m] of one source at the observation point (e, n) [km]
__device__ __forceinline__ void source_disp(const SrcConst &k, double nu, double e, double n, double &ue,
                                            double &un, double &uz)
{
    if (k.kind == 1) {
        // Mogi (1958): (1-nu)/pi * dV * (x, y, d) / R^3 ; km -> m ; volume change in slot 8
        const double de = (e - k.oe) * 1e3, dn = (n - k.on) * 1e3, d = k.dbot * 1e3;
        const double R2 = de * de + dn * dn + d * d;
        const double cf = (1.0 - nu) / 3.141592653589793 * k.U1 / (R2 * sqrt(R2));
        ue = cf * de;
        un = cf * dn;
        uz = cf * d;
        return;
    }
    const double ex = k.ex, nx = k.nx, ey = k.nx, ny = -k.ex, sd = k.sd, cd = k.cd;
    const double de = e - k.oe, dn = n - k.on;
    const double x = de * ex + dn * nx;
    const double y = -(de * ey + dn * ny);
    const double p = y * cd + k.dbot * sd;
    const double qq = y * sd - k.dbot * cd;
    const double al = 1.0 - 2.0 * nu;
    // The general expressions round like eps / |cos(dip)| (CornerSum), the vertical ones are off by ~ 5e-3 |cos(dip)|
    // slip for a dip that is not quite vertical: they cross near |cos(dip)| = 1e-7 at ~ 5e-10 slip, so a dip within
    // 5.7e-6 degrees of vertical takes the vertical I1..I5 (the geometry -- p, q, y~, d~ and the terms outside
    // I1..I5 -- keeps its cosine); DESIGN.md 3.1c
    const bool vertical = !(fabs(cd) > GEOM_VERTICAL_COS);
    const double rq = 1.0 / qq;
    CornerSum o;
    o.ssx = o.ssy = o.ssz = o.dsx = o.dsy = o.dsz = o.tfx = o.tfy = o.tfz = 0.0;
    o.i1 = o.i5 = o.k5 = o.t3 = o.i4r = 0.0;
    o.re_n = o.re_d = 1.0;
    o.dp = o.dm = 0.0;
    // f(x,p) - f(x,p-W) - f(x-L,p) + f(x-L,p-W); one corner at a time (not unrolled): the register
    // budget of one corner term lets four waves share a SIMD and hide its dependent fp64 chains
#pragma unroll 1
    for (int cn = 0; cn < 4; cn++)
        okada_corner(cn == 0 || cn == 3, (cn & 2) ? x - k.L : x, (cn & 1) ? p - k.W : p, qq, rq, sd, cd, k.rcd,
                     k.th, vertical, al, o);
    // Chinnery sums of the logarithms and of I1..I5 (eqs 28-29)
    const double S1 = log(o.re_n / o.re_d);          // sum +- ln(R + eta)
    double I1, I3, I4, I5;
    if (!vertical) {
        // sum +- [ln(R + d~) - ln(R + eta)], over cos(dip)
        const double lr = log1p((o.dp - o.dm) / (1.0 + o.dm)) * k.rcd;
        I4 = al * (lr + k.th * S1);
        I3 = al * (o.t3 + sd * k.rcd * lr - S1 * (k.th * k.rcd));
        I5 = al * 2.0 * k.rcd * (o.k5 * 1.5707963267948966 - o.i5);
        I1 = al * k.rcd * o.i1 - sd * k.rcd * I5;
    } else {
        I4 = o.i4r;
        I3 = al / 2.0 * (o.t3 - S1);
        I1 = o.i1;
        I5 = o.i5;
    }
    const double I2 = al * (-S1) - I3;
    const double ssx = o.ssx + I1 * sd, ssy = o.ssy + I2 * sd, ssz = o.ssz + I4 * sd;
    const double dsx = o.dsx - I3 * sd * cd, dsy = o.dsy - I1 * sd * cd, dsz = o.dsz - I5 * sd * cd;
    const double tfx = o.tfx - I3 * sd * sd, tfy = o.tfy - I1 * sd * sd, tfz = o.tfz - I5 * sd * sd;
    const double c2 = 1.0 / (2.0 * 3.141592653589793);
    const double ux = -k.U1 * c2 * ssx - k.U2 * c2 * dsx + k.U3 * c2 * tfx;
    const double uy = -k.U1 * c2 * ssy - k.U2 * c2 * dsy + k.U3 * c2 * tfy;
    const double uzz = -k.U1 * c2 * ssz - k.U2 * c2 * dsz + k.U3 * c2 * tfz;
    ue = ux * ex - uy * ey;
    un = ux * nx - uy * ny;
    uz = uzz;
}

}  // namespace beatamd
