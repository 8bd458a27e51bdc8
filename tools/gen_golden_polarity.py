"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/polarity.npz by running the REFERENCE's own polarity code on seeded inputs.  Needs the reference
tree (oracle/ref_import.py finds it); the fixture it writes is data (inputs and expected outputs, none of the
reference's text).

    python tools/gen_golden_polarity.py

Reference entry points exercised:
  beat/sources.py:19-40, 372-400, 403-559   MTQTSource properties (beta, gamma, theta, rot_U, lune_lambda, m9_nwu, m9),
                                            v_to_gamma, w_to_beta
  beat/heart.py:3891-4050                   radiation_weights_p / _sv / _sh, radiation_matmul
  beat/heart.py:4053-4088                   pol_synthetics (normalisation and product), driven with a stand-in source
  beat/models/distributions.py:143-173      polarity_llk, with numpy / scipy in place of the tensor module

pyrocko is not installed where this runs.  Two of its functions are replaced INSIDE THIS PROCESS: magnitude_to_moment by
a constant 1 / sqrt 2 (rho = 1; pol_synthetics normalises the scale away) and to6 by the six-vector (m00, m11, m22, m01,
m02, m12).  That order is pinned by the tree itself: calculate_radiation_weights(...).T @ to6(m9) must equal
radiation_matmul(m9, ...), which this script asserts for the three wave types.

The double couple has no in-tree formula in the reference (pyrocko's); its reference values are those of
MTQTSource(w = 0, v = 0, kappa = strike, sigma = rake, h = cos dip), which the two agree with to rounding times the
conditioning of acos at small dips (asserted below for dips above 5 degrees).

Independently, m6, the amplitudes and the likelihoods are evaluated with 50-digit mpmath arithmetic from the formulas
(mp_*).  The inputs are taken as the exact doubles they are, and so are the ARGUMENTS of the two inverse steps as the
formula forms them in float64: x = fl(3 v) for asin and u = fl(fl(3 pi / 8) - w) for the table, whose interpolation is
evaluated exactly on the float table.  (asin at |x| -> 1 and the table's ends, slope 2.5e10, are not differentiable: a
reference that rounds these arguments differently would sit 1e-8 away at v = +-1/3.)
"""
import os
import sys
from types import SimpleNamespace

import mpmath
import numpy as np
from scipy.special import erf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ref_import  # noqa: E402

ref_import.install()

from beat import heart as rheart  # noqa: E402
from beat import sources as rsources  # noqa: E402
from beat.models import distributions as rdist  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
mpmath.mp.dps = 50
mpf = mpmath.mpf
PI = np.pi
NRANDOM = 200
NSTATION = 10
# m6 for every case; amplitudes for the edge cases and the first N_AMP random ones, likelihoods for the edge cases and the
# first N_LLK (the fixture stays well under the size limit; behind m6 the kinds share one code path)
N_AMP, N_LLK = 60, 20
GAMMA = 0.2
SIGMAS = (0.05, 0.3, 2.0)
WAVES = ("any_P", "any_SV", "any_SH")


def _to6(m9):
    m9 = np.asarray(m9)
    return np.array([m9[0, 0], m9[1, 1], m9[2, 2], m9[0, 1], m9[0, 2], m9[1, 2]])


rsources.mtm.magnitude_to_moment = lambda magnitude: 1.0 / np.sqrt(2.0)
rsources.mtm.to6 = _to6
rheart.to6 = _to6
rheart.sqrt2 = np.sqrt(2.0)
rdist.tt = SimpleNamespace(erf=erf, log=np.log)


class StandIn(object):
    """what pol_synthetics asks of a source"""

    def __init__(self, m9):
        self._m9 = np.array(m9, dtype=np.float64)

    def pyrocko_moment_tensor(self):
        return SimpleNamespace(m=lambda: self._m9.copy())


def symmat(m6):
    return np.array([[m6[0], m6[3], m6[4]], [m6[3], m6[1], m6[5]], [m6[4], m6[5], m6[2]]])


# ------------------------------------------------------------------ cases
def mtqt_cases(rng):
    c38 = 3.0 * PI / 8.0
    base = (0.1, -0.05, 1.0, 0.4, 0.6)
    P = [(c38 - 3.0 / 8.0 * PI, -1.0 / 9.0, 4.0 / 5.0 * PI, -PI / 2.0, 3.0 / 4.0),       # Tape & Tape 2015 Appendix A
         (0.0, 0.0, 1.2566370614359172, -1.2566370614359172, 0.2)]                        # the example project's test value

    def with_(k, val):
        p = list(base)
        p[k] = val
        P.append(tuple(p))

    for h in (0.0, 1.0, np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0)):
        with_(4, h)
    for kap in (0.0, 2.0 * PI, np.nextafter(2.0 * PI, 0.0)):
        with_(2, kap)
    for sg in (PI / 2.0, -PI / 2.0, np.nextafter(PI / 2.0, 0.0), np.nextafter(-PI / 2.0, 0.0)):
        with_(3, sg)
    for v in (1.0 / 3.0, -1.0 / 3.0, np.nextafter(1.0 / 3.0, 0.0), np.nextafter(-1.0 / 3.0, 0.0)):
        with_(1, v)
    for w in (c38, -c38, np.nextafter(c38, 0.0), np.nextafter(-c38, 0.0)):
        with_(0, w)
    # exact table nodes: w with fl(c38 - w) == U_MAPPING[j]
    nodes = 0
    for j in (1, 2, 17, 250, 499, 500, 777, 997, 998):
        w = c38 - rsources.U_MAPPING[j]
        if c38 - w == rsources.U_MAPPING[j]:
            with_(0, w)
            nodes += 1
    assert nodes >= 3, nodes
    n_edge = len(P)
    for _ in range(NRANDOM):
        P.append((rng.uniform(-c38, c38), rng.uniform(-1.0 / 3.0, 1.0 / 3.0), rng.uniform(0.0, 2.0 * PI),
                  rng.uniform(-PI / 2.0, PI / 2.0), rng.uniform(0.0, 1.0)))
    return np.array(P, dtype=np.float64), n_edge


def mt_cases(rng):
    P = [np.eye(6)[k] for k in range(6)] + [-np.eye(6)[0], np.ones(6), np.array([1.0, 1.0, 1.0, 0, 0, 0]),
                                             np.array([1e-100, 0, 0, 0, 2e-100, 0]), np.array([1e100, -1e100, 0, 3e99, 0, 0])]
    n_edge = len(P)
    P += [rng.uniform(-1.0, 1.0, 6) for _ in range(NRANDOM)]
    return np.array(P, dtype=np.float64), n_edge


def dc_cases(rng):
    P = [(0.0, 45.0, 0.0), (360.0, 45.0, 90.0), (120.0, 90.0, -90.0), (30.0, 5.0, 180.0), (30.0, 60.0, -180.0), (271.0, 89.999, 0.5)]
    n_edge = len(P)
    P += [(rng.uniform(0.0, 360.0), rng.uniform(5.0, 90.0), rng.uniform(-180.0, 180.0)) for _ in range(NRANDOM)]
    return np.array(P, dtype=np.float64), n_edge


# ------------------------------------------------------------------ mpmath
def mp_rot(axis, a):
    c, s = mpmath.cos(a), mpmath.sin(a)
    if axis == "x":
        return mpmath.matrix([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == "y":
        return mpmath.matrix([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return mpmath.matrix([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def mp_interp(x, xp, fp):
    """the piecewise-linear interpolant of the float table, evaluated exactly at the float x"""
    n = xp.size
    if x < xp[0]:
        return mpf(fp[0])
    if x > xp[n - 1]:
        return mpf(fp[n - 1])
    j = int(np.searchsorted(xp, x, side="right")) - 1
    if j == n - 1 or xp[j] == x:
        return mpf(fp[j])
    return (mpf(fp[j + 1]) - mpf(fp[j])) / (mpf(xp[j + 1]) - mpf(xp[j])) * (mpf(x) - mpf(xp[j])) + mpf(fp[j])


def mp_normalise(m9):
    ssq = sum(m9[i, j] ** 2 for i in range(3) for j in range(3))
    scale = mpmath.sqrt(ssq) / mpmath.sqrt(2)
    return [m9[0, 0] / scale, m9[1, 1] / scale, m9[2, 2] / scale, m9[0, 1] / scale, m9[0, 2] / scale, m9[1, 2] / scale]


def mp_mtqt(p):
    w, v, kappa, sigma, h = [float(x) for x in p]
    gamma = mpmath.asin(mpf(3.0 * v)) / 3
    beta = mp_interp(3.0 * PI / 8.0 - w, rsources.U_MAPPING, rsources.BETA_MAPPING)
    theta = mpmath.acos(mpf(h))
    sb, cb, sg, cg = mpmath.sin(beta), mpmath.cos(beta), mpmath.sin(gamma), mpmath.cos(gamma)
    s2, s3, s6 = mpmath.sqrt(2), mpmath.sqrt(3), mpmath.sqrt(6)
    vec = mpmath.matrix([sb * cg, sb * sg, cb])
    lam = mpmath.matrix([[s3, -1, s2], [0, 2, s2], [-s3, -1, s2]]) * vec / s6
    U = mp_rot("z", -mpf(kappa)) * mp_rot("x", theta) * mp_rot("z", mpf(sigma)) * mp_rot("y", -mpmath.pi / 4)
    m_nwu = U * mpmath.diag([lam[0], lam[1], lam[2]]) * U.T
    R = mpmath.diag([1, -1, -1])
    return mp_normalise(R * m_nwu * R.T)


def mp_dc(p):
    ph, de, la = [mpmath.radians(mpf(float(x))) for x in p]
    sp, cp, sd, cd, sl, cl = mpmath.sin(ph), mpmath.cos(ph), mpmath.sin(de), mpmath.cos(de), mpmath.sin(la), mpmath.cos(la)
    s2p, c2p, s2d, c2d = mpmath.sin(2 * ph), mpmath.cos(2 * ph), mpmath.sin(2 * de), mpmath.cos(2 * de)
    m6 = [-(sd * cl * s2p + s2d * sl * sp * sp), sd * cl * s2p - s2d * sl * cp * cp, s2d * sl,
          sd * cl * c2p + s2d * sl * s2p / 2, -(cd * cl * cp + c2d * sl * sp), -(cd * cl * sp - c2d * sl * cp)]
    return mp_normalise(mpmath.matrix([[m6[0], m6[3], m6[4]], [m6[3], m6[1], m6[5]], [m6[4], m6[5], m6[2]]]))


def mp_mt(p):
    m6 = [mpf(float(x)) for x in p]
    return mp_normalise(mpmath.matrix([[m6[0], m6[3], m6[4]], [m6[3], m6[1], m6[5]], [m6[4], m6[5], m6[2]]]))


def mp_amplitudes(rw, m6):
    return [sum(mpf(rw[k, s]) * m6[k] for k in range(6)) for s in range(rw.shape[1])]


def mp_llk(obs, amp, gamma, sigma):
    out = []
    g, sg = mpf(gamma), mpf(sigma)
    for o, a in zip(obs, amp):
        p = g + (1 - 2 * g) * (mpf(1) / 2 + mpmath.erf(a / sg / mpmath.sqrt(2)) / 2)
        out.append((1 + mpf(float(o))) / 2 * mpmath.log(p) + (1 - mpf(float(o))) / 2 * mpmath.log(1 - p))
    return out


def to_f(xs):
    return np.array([float(x) for x in xs])


# ------------------------------------------------------------------ main
def main():
    rng = np.random.RandomState(20240911)
    out = dict(gamma=np.float64(GAMMA), sigmas=np.array(SIGMAS), u_mapping=rsources.U_MAPPING, beta_mapping=rsources.BETA_MAPPING)
    # stations: takeoff angles over [0, pi] (both ends, above pi/2 too), azimuths over [0, 2 pi)
    takeoff = np.concatenate([[0.0, PI, PI / 2.0, 0.3, 2.8], rng.uniform(0.0, PI, NSTATION - 5)])
    azimuth = np.concatenate([[0.0, np.nextafter(2.0 * PI, 0.0), PI, 1.0, 5.5], rng.uniform(0.0, 2.0 * PI, NSTATION - 5)])
    obs = rng.choice(np.array([-1, 1], dtype=np.int16), size=3 * NSTATION)
    obs[[3, 17]] = 0
    out.update(takeoff=takeoff, azimuth=azimuth, obs=obs, wavenames=np.array(WAVES))
    rws = [rheart.calculate_radiation_weights(takeoff, azimuth, w) for w in WAVES]
    for w, r, f in zip(WAVES, rws, (rheart.radiation_weights_p, rheart.radiation_weights_sv, rheart.radiation_weights_sh)):
        assert np.array_equal(r, f(takeoff, azimuth))
        out["rw_" + w] = r
    rw = np.concatenate(rws, axis=1)

    P, n_edge = {}, {}
    P["mtqt"], n_edge["mtqt"] = mtqt_cases(rng)
    P["mt"], n_edge["mt"] = mt_cases(rng)
    P["dc"], n_edge["dc"] = dc_cases(rng)

    # reference sources -> m9 (unnormalised) per case
    m9s = {"mtqt": [], "mt": [], "dc": []}
    props = {k: [] for k in ("beta", "gamma", "theta", "rot_U", "lune_lambda", "m9_nwu", "m9")}
    for p in P["mtqt"]:
        s = rsources.MTQTSource(w=p[0], v=p[1], kappa=p[2], sigma=p[3], h=p[4], magnitude=1.0)
        assert abs(s.rho - 1.0) < 1e-15
        for k in props:
            props[k].append(np.array(getattr(s, k), dtype=np.float64))
        m9s["mtqt"].append(s.m9)
        assert np.array_equal(s.m6, _to6(s.m9))
    for k, v in props.items():
        out["mtqt_" + k] = np.array(v)
    out["w_to_beta_w"] = P["mtqt"][:, 0].copy()
    out["w_to_beta"] = np.array([rsources.w_to_beta(w, u_mapping=rsources.U_MAPPING, beta_mapping=rsources.BETA_MAPPING)
                                 for w in P["mtqt"][:, 0]])
    out["v_to_gamma"] = np.array([rsources.v_to_gamma(v) for v in P["mtqt"][:, 1]])
    for p in P["mt"]:
        m9s["mt"].append(symmat(p))
    for p in P["dc"]:
        s = rsources.MTQTSource(w=0.0, v=0.0, kappa=np.deg2rad(p[0]), sigma=np.deg2rad(p[2]), h=np.cos(np.deg2rad(p[1])),
                                magnitude=1.0)
        m9s["dc"].append(s.m9)

    # the six-vector order is pinned by the tree: weights == matmul
    mm = []
    for i in (0, 1, n_edge["mtqt"], n_edge["mtqt"] + 7):
        m9 = m9s["mtqt"][i]
        row = []
        for w, r in zip(WAVES, rws):
            a = rheart.radiation_matmul(m9, takeoff, azimuth, w)
            assert np.max(np.abs(r.T.dot(_to6(m9)) - a)) < 4e-16, w
            row.append(a)
        mm.append(np.concatenate(row))
    out["matmul_cases"] = np.array([0, 1, n_edge["mtqt"], n_edge["mtqt"] + 7])
    out["matmul"] = np.array(mm)

    mp_fun = {"mtqt": mp_mtqt, "mt": mp_mt, "dc": mp_dc}
    for kind in ("mtqt", "mt", "dc"):
        n = P[kind].shape[0]
        ref_m6, ref_amp, mp_m6, mp_amp = [], [], [], []
        n_amp, n_llk = n_edge[kind] + N_AMP, n_edge[kind] + N_LLK
        ref_ll = np.empty((len(SIGMAS), n_llk, rw.shape[1]))
        mp_ll = np.empty_like(ref_ll)
        for i in range(n):
            src = StandIn(m9s[kind][i])
            amp = rheart.pol_synthetics(src, radiation_weights=rw)                      # heart.py:4086-4088
            m9n = src._m9 / (np.sqrt(np.sum(src._m9 ** 2)) / np.sqrt(2.0))
            ref_m6.append(_to6(m9n))
            tm6 = mp_fun[kind](P[kind][i])
            mp_m6.append(to_f(tm6))
            if i >= n_amp:
                continue
            ref_amp.append(amp)
            tamp = mp_amplitudes(rw, tm6)
            mp_amp.append(to_f(tamp))
            for k, sg in enumerate(SIGMAS if i < n_llk else ()):
                ref_ll[k, i] = rdist.polarity_llk(obs.astype(np.float64), amp, GAMMA, sg)
                mp_ll[k, i] = to_f(mp_llk(obs, tamp, GAMMA, sg))
        ref_m6, ref_amp, mp_m6, mp_amp = (np.array(a) for a in (ref_m6, ref_amp, mp_m6, mp_amp))
        out.update({"P_" + kind: P[kind], "n_edge_" + kind: np.int64(n_edge[kind]), "ref_m6_" + kind: ref_m6,
                    "ref_amp_" + kind: ref_amp, "mp_m6_" + kind: mp_m6, "mp_amp_" + kind: mp_amp, "ref_llk_" + kind: ref_ll,
                    "mp_llk_" + kind: mp_ll})
        # the reference's own distance from the mpmath values, in units of 2^-53
        out["ref_m6_units_" + kind] = np.float64(np.max(np.abs(ref_m6 - mp_m6)) * 2.0 ** 53)
        print("%-4s %d cases (%d edge): reference m6 %.2f units of 2^-53 from mpmath, amplitudes %.3g, llk %.3g absolute"
              % (kind, n, n_edge[kind], out["ref_m6_units_" + kind], np.max(np.abs(ref_amp - mp_amp)),
                 np.max(np.abs(ref_ll - mp_ll))))
    if not os.path.isdir(GOLDEN):
        os.makedirs(GOLDEN)
    path = os.path.join(GOLDEN, "polarity.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
