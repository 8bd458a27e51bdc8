// mechanism.hpp -- the per-draw arithmetic behind the mechanism-ensemble figures (beat/plotting/seismic.py:1334-1425
// mts2amps, :1664-1850 fuzzy_mt_decomposition, :2183-2310 draw_hudson), stated once as plain __host__ __device__ functions:
// k_mt_decompose (mechanisms.hip) and a host program (tests/test_mechanisms_host.py) compile the same text.  No
// contraction, no fma(): every product and sum rounds once, in the order written.
//
// A tensor is (mnn, mee, mdd, mne, mnd, med), north-east-down; symmat6 lays it out as
//     [[mnn, mne, mnd], [mne, mee, med], [mnd, med, mdd]].
//
// UNVERIFIED RESTATEMENTS (pyrocko is not available to this project's tests; the rules below are written from memory of
// its published source and pinned only to multi-precision evaluations of themselves):
//   * mech_standard_decomposition: pyrocko.moment_tensor.MomentTensor.standard_decomposition;
//   * mech_hudson: the (u, v) of Hudson, Pearce & Rogers (1989, JGR 94, 765-774) with T = 2 m2' / D; whether the sign of u
//     agrees with pyrocko.plot.hudson.project has not been checked.
#ifndef BEATAMD_MECHANISM_HPP
#define BEATAMD_MECHANISM_HPP

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MECH_HD __host__ __device__ inline
#else
#define MECH_HD inline
#endif

namespace beatamd {

constexpr int MECH_NPART = 5;            // iso, dc, clvd, dev, full
constexpr int MECH_JACOBI_SWEEPS = 32;   // cap; a 3 x 3 matrix is done after 5 to 8

// Aki & Richards (1980, box 4.4): the unit double couple of (strike, dip, rake) [deg]
MECH_HD void mech_dc_m6(double strike, double dip, double rake, double *m)
{
#pragma clang fp contract(off)
    const double d2r = 3.14159265358979323846 / 180.0;
    const double ph = strike * d2r, de = dip * d2r, la = rake * d2r;
    const double sp = sin(ph), cp = cos(ph), sd = sin(de), cd = cos(de), sl = sin(la), cl = cos(la);
    const double s2p = 2.0 * (sp * cp), c2p = cp * cp - sp * sp, s2d = 2.0 * (sd * cd), c2d = cd * cd - sd * sd;
    m[0] = -((sd * cl) * s2p + (s2d * sl) * (sp * sp));
    m[1] = (sd * cl) * s2p - (s2d * sl) * (cp * cp);
    m[2] = s2d * sl;
    m[3] = (sd * cl) * c2p + (0.5 * (s2d * sl)) * s2p;
    m[4] = -((cd * cl) * cp + (c2d * sl) * sp);
    m[5] = -((cd * cl) * sp - (c2d * sl) * cp);
}

// one Jacobi rotation in the (p, q) plane of the symmetric a (diagonal d[3], off-diagonals o[3] = a01, a02, a12) that
// zeroes a_pq; r is the third index; opq, orp, orq index o.  V [3][3] collects the rotations (columns = eigenvectors).
MECH_HD void mech_rotate(double *d, double *o, double (*V)[3], int p, int q, int opq, int orp, int orq, bool late)
{
#pragma clang fp contract(off)
    const double apq = o[opq];
    if (apq == 0.0) return;
    const double g = 100.0 * fabs(apq);
    // past the first sweeps an off-diagonal that no longer changes either diagonal entry is rounding noise
    if (late && fabs(d[p]) + g == fabs(d[p]) && fabs(d[q]) + g == fabs(d[q])) {
        o[opq] = 0.0;
        return;
    }
    const double h = d[q] - d[p];
    double t;
    if (fabs(h) + g == fabs(h)) {
        t = apq / h;   // tan of a tiny angle; theta^2 would overflow
    } else {
        const double theta = 0.5 * h / apq;
        t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
        if (theta < 0.0) t = -t;
    }
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
    const double hh = t * apq;
    d[p] = d[p] - hh;
    d[q] = d[q] + hh;
    o[opq] = 0.0;
    const double arp = o[orp], arq = o[orq];
    o[orp] = arp - s * (arq + arp * tau);
    o[orq] = arq + s * (arp - arq * tau);
    for (int k = 0; k < 3; k++) {
        const double vp = V[k][p], vq = V[k][q];
        V[k][p] = vp - s * (vq + vp * tau);
        V[k][q] = vq + s * (vp - vq * tau);
    }
}

// orders three (key, value, column of V) triples by key ascending with compare-exchanges at fixed positions (0,1), (1,2),
// (0,1); only a strictly smaller key moves ahead, so equal keys keep their order
MECH_HD void mech_cmpx3(double *key, double *val, double (*V)[3], int a, int b)
{
    if (key[b] < key[a]) {
        double t = key[a]; key[a] = key[b]; key[b] = t;
        t = val[a]; val[a] = val[b]; val[b] = t;
        for (int k = 0; k < 3; k++) {
            t = V[k][a]; V[k][a] = V[k][b]; V[k][b] = t;
        }
    }
}
MECH_HD void mech_sort3(double *key, double *val, double (*V)[3])
{
    mech_cmpx3(key, val, V, 0, 1);
    mech_cmpx3(key, val, V, 1, 2);
    mech_cmpx3(key, val, V, 0, 1);
}

// eigen-decomposition of symmat6(m): cyclic Jacobi rotations, at most MECH_JACOBI_SWEEPS sweeps, done when the three
// off-diagonals are exact zeros (a diagonal input leaves at once, its eigenvectors the unit vectors).  w [3] ascending
// (equal eigenvalues keep the order of their columns), V [3][3]: column j is the eigenvector of w[j].
MECH_HD void mech_eig3(const double *m, double *w, double (*V)[3])
{
#pragma clang fp contract(off)
    double d[3] = {m[0], m[1], m[2]};
    double o[3] = {m[3], m[4], m[5]};   // a01, a02, a12
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < MECH_JACOBI_SWEEPS; sweep++) {
        if (o[0] == 0.0 && o[1] == 0.0 && o[2] == 0.0) break;
        const bool late = sweep >= 3;
        mech_rotate(d, o, V, 0, 1, 0, 1, 2, late);   // r = 2: a20 = o[1], a21 = o[2]
        mech_rotate(d, o, V, 0, 2, 1, 0, 2, late);   // r = 1: a10 = o[0], a12 = o[2]
        mech_rotate(d, o, V, 1, 2, 2, 0, 1, late);   // r = 0: a01 = o[0], a02 = o[1]
    }
    for (int j = 0; j < 3; j++) w[j] = d[j];
    mech_sort3(d, w, V);
}

// the tensor mts2amps multiplies (seismic.py:1410-1417): m9 / (sqrt(sum m9^2) / sqrt 2) over all nine entries, as six.
// An all-zero part gives 0 / 0 = NaN, as numpy does; the count kernel adds nothing for it.
MECH_HD void mech_unit6(const double *m, double *u)
{
#pragma clang fp contract(off)
    const double ssq = ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) + 2.0 * ((m[3] * m[3] + m[4] * m[4]) + m[5] * m[5]);
    const double scale = sqrt(ssq) / 1.4142135623730951;
    for (int k = 0; k < 6; k++) u[k] = m[k] / scale;
}

// MomentTensor.standard_decomposition as fuzzy_mt_decomposition reads it (seismic.py:1689-1696); the order of the five
// is iso, dc, clvd, dev, full.  moments [5], ratios [5] (moment_x / moment, 1 for the full tensor), parts [5][6].
MECH_HD void mech_standard_decomposition(const double *m, double *moments, double *ratios, double (*parts)[6])
{
#pragma clang fp contract(off)
    const double iso = ((m[0] + m[1]) + m[2]) / 3.0;
    const double moment_iso = fabs(iso);
    const double dev[6] = {m[0] - iso, m[1] - iso, m[2] - iso, m[3], m[4], m[5]};
    double e[3], V[3][3];
    mech_eig3(dev, e, V);
    // by |e| ascending, stable
    double key[3] = {fabs(e[0]), fabs(e[1]), fabs(e[2])};
    mech_sort3(key, e, V);
    const double e0 = e[0], e2 = e[2];
    const double moment_dev = fabs(e2);
    const double moment = moment_iso + moment_dev;
    double signed_dc = 0.0;
    if (!(moment_dev < 1e-6 * moment_iso)) {
        const double r = e0 / e2;
        signed_dc = e2 * (1.0 + 2.0 * (r < 0.0 ? r : 0.0));
    }
    const double moment_dc = fabs(signed_dc);
    const int ia[6] = {0, 1, 2, 0, 0, 1}, ib[6] = {0, 1, 2, 1, 2, 2};
    for (int k = 0; k < 6; k++) {
        const double dc = signed_dc * (V[ia[k]][2] * V[ib[k]][2] - V[ia[k]][1] * V[ib[k]][1]);
        parts[0][k] = k < 3 ? iso : 0.0;
        parts[1][k] = dc;
        parts[2][k] = dev[k] - dc;
        parts[3][k] = dev[k];
        parts[4][k] = m[k];
    }
    moments[0] = moment_iso;
    moments[1] = moment_dc;
    moments[2] = moment_dev - moment_dc;
    moments[3] = moment_dev;
    moments[4] = moment;
    for (int k = 0; k < 4; k++) ratios[k] = moments[k] / moment;
    ratios[4] = 1.0;
}

// Hudson, Pearce & Rogers (1989): (u, v) of the source-type plot from the eigenvalues w [3] ASCENDING of the full tensor
MECH_HD void mech_hudson(const double *w, double *uv)
{
#pragma clang fp contract(off)
    const double m1 = w[2], m2 = w[1], m3 = w[0];
    const double iso = ((m1 + m2) + m3) / 3.0;
    const double d1 = m1 - iso, d2 = m2 - iso, d3 = m3 - iso;
    const double D = fabs(d1) > fabs(d3) ? fabs(d1) : fabs(d3);
    const double k = iso / (fabs(iso) + D);
    const double T = D == 0.0 ? 0.0 : 2.0 * d2 / D;
    const double tau = T * (1.0 - fabs(k));
    double den = 1.0;
    if (tau > 0.0 && k > 0.0) den = tau < 4.0 * k ? 1.0 - tau / 2.0 : 1.0 - 2.0 * k;
    else if (tau < 0.0 && k < 0.0) den = tau > 4.0 * k ? 1.0 + tau / 2.0 : 1.0 + 2.0 * k;
    uv[0] = tau / den;
    uv[1] = k / den;
}

// everything k_mt_decompose writes for one draw
struct MechDraw {
    double evals[3], evecs[3][3];
    double moments[MECH_NPART], ratios[MECH_NPART], parts[MECH_NPART][6], unit[MECH_NPART][6], uv[2];
};

MECH_HD void mech_draw(const double *m, MechDraw &r)
{
    mech_eig3(m, r.evals, r.evecs);
    mech_standard_decomposition(m, r.moments, r.ratios, r.parts);
    for (int p = 0; p < MECH_NPART; p++) mech_unit6(r.parts[p], r.unit[p]);
    mech_hudson(r.evals, r.uv);
}

}  // namespace beatamd
#endif
