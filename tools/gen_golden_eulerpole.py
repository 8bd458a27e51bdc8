"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/euler_pole.npz by running the REFERENCE's own Euler-pole code (numpy ``point`` branch) on seeded
inputs.  Needs the reference tree (oracle/ref_import.py finds it); the fixture it writes is data (inputs and expected
outputs, none of the reference's text).

    python tools/gen_golden_eulerpole.py

Reference entry points exercised:
  beat/config.py:840-853               EulerPoleConfig(dataset_names, enabled).init_correction()
  beat/models/corrections.py:90-140    EulerPoleCorrection.setup_correction / get_displacements(point=...)
  beat/heart.py:4326-4392              velocities_from_pole(..., earth_shape="ellipsoid")
  beat/ffi/fault.py:1497, 1500-1517    the |sum| of euler_pole2slips, backslip2coupling
Coefficient ranges: pole_lat +-90, pole_lon +-180, omega +-10 deg / Myr (beat/defaults.py), plus forced sets: poles at
+-90 latitude, at +-180 longitude, within 1e-3 deg of a station, omega = 0 and omega < 0.

pyrocko is not installed where this runs: ``heart.orthodrome`` is replaced INSIDE THIS PROCESS by a namespace with
``earthradius`` and a ``geodetic_to_ecef`` of the textbook closed form (beat_amd's EarthModel, with the three
constants recorded in the fixture), so that the reference's own cross product, ``cartesian_to_local``, einsum, mask and
line-of-sight projection produce the numbers.  Independently of both, the correction and the three derived
coefficients are evaluated with 50-digit mpmath arithmetic from the formulas alone (mp_*).
"""
import os
import sys
from types import SimpleNamespace

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ref_import  # noqa: E402

ref_import.install()

from beat import heart  # noqa: E402
from beat.config import EulerPoleConfig  # noqa: E402
from beat.ffi.fault import backslip2coupling  # noqa: E402

from beat_amd.models.corrections import EarthModel  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NSETS = 12
NPATCH = 65
mpmath.mp.dps = 50


def mp_ecef(lat, lon, earth):
    r, a, f = [mpmath.mpf(v) for v in earth]
    e2 = 2 * f - f * f
    la, lo = mpmath.radians(mpmath.mpf(lat)), mpmath.radians(mpmath.mpf(lon))
    N = a / mpmath.sqrt(1 - e2 * mpmath.sin(la) ** 2)
    return [N * mpmath.cos(la) * mpmath.cos(lo) / r, N * mpmath.cos(la) * mpmath.sin(lo) / r,
            N * (1 - e2) * mpmath.sin(la) / r]


def mp_coefficients(plat, plon, omega, earth):
    p = mp_ecef(plat, plon, earth)
    w = mpmath.mpf(omega) * mpmath.mpf("1e-6") * mpmath.pi / 180 * mpmath.mpf(earth[0])
    return [w * v for v in p]


def mp_correction(lats, lons, los, mask, coef, earth):
    out = np.zeros(lats.size)
    for i in range(lats.size):
        if mask[i]:
            continue
        x = mp_ecef(lats[i], lons[i], earth)
        v = [coef[1] * x[2] - coef[2] * x[1], coef[2] * x[0] - coef[0] * x[2], coef[0] * x[1] - coef[1] * x[0]]
        la, lo = mpmath.radians(mpmath.mpf(lats[i])), mpmath.radians(mpmath.mpf(lons[i]))
        sl, cl, so, co = mpmath.sin(la), mpmath.cos(la), mpmath.sin(lo), mpmath.cos(lo)
        T = [[-sl * co, -sl * so, cl], [-so, co, 0], [-cl * co, -cl * so, -sl]]
        neu = [sum(T[j][m] * v[m] for m in range(3)) for j in range(3)]
        out[i] = float(sum(mpmath.mpf(los[i, j]) * neu[j] for j in range(3)))
    return out


def main():
    rng = np.random.default_rng(20261019)
    em = EarthModel(EarthModel.RADIUS, EarthModel.EQUATOR_RADIUS, EarthModel.OBLATENESS)
    earth = np.array(em.as_tuple())
    nsta, ncomp = 24, 3
    n = nsta * ncomp
    sta_lat = rng.uniform(-44.0, -38.0, nsta)
    sta_lon = rng.uniform(170.0, 178.0, nsta)
    lats, lons = np.repeat(sta_lat, ncomp), np.repeat(sta_lon, ncomp)
    los0 = np.tile(np.eye(3), (nsta, 1))
    los1 = rng.normal(size=(n, 3))
    los1 /= np.linalg.norm(los1, axis=1)[:, None]
    sta_mask = np.zeros(nsta, dtype=bool)
    sta_mask[[2, 7, 19]] = True
    mask = np.repeat(sta_mask, ncomp)

    coefs = np.stack([rng.uniform(-90.0, 90.0, NSETS), rng.uniform(-180.0, 180.0, NSETS),
                      rng.uniform(-10.0, 10.0, NSETS)], axis=1)
    forced = np.array([[90.0, 12.0, 1.5], [-90.0, -47.0, 0.8], [-61.3, 180.0, 2.1], [33.0, -180.0, 0.4],
                       [sta_lat[5] + 7e-4, sta_lon[5] - 5e-4, 3.0], [-40.0, 175.0, 0.0], [-62.0, 174.0, -0.9]])
    coefs = np.concatenate([coefs, forced])
    ns = coefs.shape[0]

    def geodetic_to_ecef(lat, lon, alt):
        assert np.all(np.asarray(alt) == 0.0)
        return em.geodetic_to_ecef(lat, lon)

    out = {"note": np.array(
        "lats/lons [deg] of 24 stations x 3 components; los0: unit axes (N, E, U), los1: oblique; mask over whole "
        "stations; coefs (pole_lat, pole_lon, omega): 12 seeded sets, then forced ones (poles at +-90 lat, +-180 lon, "
        "within 1e-3 deg of station 5, omega = 0, omega < 0). disp*: the reference's EulerPoleCorrection."
        "get_displacements(point=...) with heart.orthodrome replaced by (earthradius, closed-form geodetic_to_ecef) of "
        "the recorded earth constants (radius, equator radius, oblateness). mp_*: 50-digit mpmath values of the "
        "formulas. patch_*: seeded patch centres, strike vectors (ENU), back-slips; euler_slips / coupling: "
        "|sum(velocities_from_pole * strikevectors_neu)| and backslip2coupling of the reference.")}
    real = heart.orthodrome
    heart.orthodrome = SimpleNamespace(earthradius=em.radius, geodetic_to_ecef=geodetic_to_ecef)
    try:
        for b, lv in enumerate((los0, los1)):
            cfg = EulerPoleConfig(dataset_names=["gnss"], enabled=True)
            corr = cfg.init_correction()
            corr.setup_correction(locy=lats, locx=lons, los_vector=lv, data_mask=mask, dataset_name="gnss", number=b)
            assert list(corr.correction_names) == ["%d_%s" % (b, s) for s in ("pole_lat", "pole_lon", "omega")]
            disp = np.empty((ns, n))
            mp_disp = np.empty((ns, n))
            for i in range(ns):
                point = dict(zip(corr.correction_names, coefs[i]))
                disp[i] = corr.get_displacements({}, point=point)
                mp_disp[i] = mp_correction(lats, lons, lv, mask, mp_coefficients(*coefs[i], earth), earth)
            out["los%d" % b] = lv
            out["disp%d" % b] = disp
            out["mp_disp%d" % b] = mp_disp
        out["mp_coef"] = np.array([[float(v) for v in mp_coefficients(*c, earth)] for c in coefs])

        # coupling: fault.py:1478-1480, 1488-1497, 1500-1517 on seeded patches
        plats = rng.uniform(-43.0, -39.0, NPATCH)
        plons = rng.uniform(172.0, 177.0, NPATCH)
        strike = rng.uniform(0.0, 2 * np.pi, NPATCH)
        sv_enu = np.stack([np.sin(strike), np.cos(strike), np.zeros(NPATCH)], axis=1)
        sv_neu = np.zeros_like(sv_enu)
        sv_neu[:, 0] = sv_enu[:, 1]
        sv_neu[:, 1] = sv_enu[:, 0]
        uparr = rng.uniform(-0.01, 0.06, (ns, NPATCH))
        uparr[:, 3] = 0.0
        es = np.empty((ns, NPATCH))
        cp = np.empty((ns, NPATCH))
        with np.errstate(divide="ignore", invalid="ignore"):
            for i in range(ns):
                v = heart.velocities_from_pole(lats=plats, lons=plons, pole_lat=coefs[i, 0], pole_lon=coefs[i, 1],
                                               omega=coefs[i, 2], earth_shape="ellipsoid")
                es[i] = np.abs((v * sv_neu).sum(axis=1))
                cp[i] = backslip2coupling({"uparr": uparr[i].copy()}, es[i])
    finally:
        heart.orthodrome = real
    out.update({"lats": lats, "lons": lons, "mask": mask, "coefs": coefs, "earth": earth, "patch_lats": plats,
                "patch_lons": plons, "patch_strikevectors_enu": sv_enu, "patch_uparr": uparr, "euler_slips": es,
                "coupling": cp})
    path = os.path.join(GOLDEN, "euler_pole.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f kB)" % (path, os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
