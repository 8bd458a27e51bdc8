"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/geo_corrections.npz by running the REFERENCE's own correction classes (numpy ``point`` branch)
on seeded inputs.  Needs the reference tree (oracle/ref_import.py finds it), so it runs where that tree is mounted;
the fixture it writes is data (inputs and expected outputs, none of the reference's text).

    python tools/gen_golden_corrections.py

Reference entry points exercised:
  beat/config.py:872-892        RampConfig(dataset_names, enabled).init_correction()
  beat/models/corrections.py:46-87   RampCorrection.setup_correction / get_displacements(point=...)
  beat/heart.py:4494-4512       get_ramp_displacement
  beat/config.py:856-869        StrainRateConfig(...).init_correction()
  beat/models/corrections.py:143-205  StrainRateCorrection.setup_correction / get_displacements(point=...)
  beat/heart.py:4441-4491       velocities_from_strain_rate_tensor
Coefficient ranges: the physical bounds of beat/defaults.py:244-249 (ramps +-0.1, offset +-0.05 m) and :167-...
(strain-rate components +-200 nanostrain).

Local coordinates.  The pickled Laquila scenes hold lons / lats only (east_shifts / north_shifts are None there; the
reference derives them through pyrocko at set-up, heart.py:1127-1143): the fixture records seeded coordinates over
+-30 km in metres instead -- the ramp arithmetic does not depend on where the coordinates came from.  For the strain
rate, ``heart.orthodrome`` is replaced INSIDE THIS PROCESS by a namespace whose ``geographic_midpoint`` /
``latlon_to_ne_numpy`` return the recorded local coordinates, so that the reference's own ``D.dot(nes)``, station
mask and line-of-sight projection produce the numbers.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402

ref_import.install()

from beat import heart  # noqa: E402
from beat.config import RampConfig, StrainRateConfig  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NSETS = 12


def gen_ramp(out, rng):
    laq = np.load(os.path.join(GOLDEN, "laquila_geodetic.npz"))
    names = ["scene_%d" % d for d in range(int(laq["n"]))]
    cfg = RampConfig(dataset_names=names, enabled=True)
    for d, name in enumerate(names):
        data, odw = laq["d%d_displacement" % d], laq["d%d_odw" % d]
        n = data.size
        east = rng.uniform(-30e3, 30e3, n)
        north = rng.uniform(-30e3, 30e3, n)
        corr = cfg.init_correction()
        corr.setup_correction(locy=north, locx=east, los_vector=None, data_mask=None, dataset_name=name)
        assert list(corr.correction_names) == ["%s_%s" % (name, s) for s in ("azimuth_ramp", "range_ramp", "offset")]
        coefs = np.stack([rng.uniform(-0.1, 0.1, NSETS), rng.uniform(-0.1, 0.1, NSETS),
                          rng.uniform(-0.05, 0.05, NSETS)], axis=1)
        mu = rng.normal(0.0, 0.05, (NSETS, n))
        disp = np.empty((NSETS, n))
        res = np.empty((NSETS, n))
        for i in range(NSETS):
            point = dict(zip(corr.correction_names, coefs[i]))
            disp[i] = corr.get_displacements({}, point=point)
            res[i] = (data - mu[i]) * odw - disp[i]
        out.update({"ramp%d_east_shifts" % d: east, "ramp%d_north_shifts" % d: north, "ramp%d_coefs" % d: coefs,
                    "ramp%d_mu" % d: mu, "ramp%d_disp" % d: disp, "ramp%d_res" % d: res,
                    "ramp%d_data" % d: data, "ramp%d_odw" % d: odw})
    out["ramp_names"] = np.array(names)
    out["ramp_n"] = np.array(len(names))


def gen_strain(out, rng):
    nsta, ncomp = 24, 3
    n = nsta * ncomp
    # one row per (station, component): coordinates repeated per component, unit vectors of the component axes
    # (north, east, up) as line-of-sight vectors, a station mask over whole stations
    sta_n = rng.uniform(-80e3, 80e3, nsta)
    sta_e = rng.uniform(-80e3, 80e3, nsta)
    norths, easts = np.repeat(sta_n, ncomp), np.repeat(sta_e, ncomp)
    los = np.tile(np.eye(3), (nsta, 1))
    # a second block: oblique line-of-sight vectors (the projection mixes both components)
    los2 = rng.normal(size=(n, 3))
    los2 /= np.linalg.norm(los2, axis=1)[:, None]
    sta_mask = np.zeros(nsta, dtype=bool)
    sta_mask[[2, 7, 19]] = True
    mask = np.repeat(sta_mask, ncomp)
    lats = 42.0 + norths / 111e3        # placeholders: the reprojection is replaced below
    lons = 13.0 + easts / 80e3

    real = heart.orthodrome
    heart.orthodrome = SimpleNamespace(
        geographic_midpoint=lambda la, lo: (42.0, 13.0),
        latlon_to_ne_numpy=lambda mla, mlo, la, lo: (norths, easts))
    try:
        coefs = rng.uniform(-200.0, 200.0, (NSETS, 4))
        for b, lv in enumerate((los, los2)):
            cfg = StrainRateConfig(dataset_names=["gnss"], enabled=True)
            corr = cfg.init_correction()
            corr.setup_correction(locy=lats, locx=lons, los_vector=lv, data_mask=mask, dataset_name="gnss", number=b)
            assert list(corr.correction_names) == ["%d_%s" % (b, s) for s in ("exx", "eyy", "exy", "rotation")]
            disp = np.empty((NSETS, n))
            for i in range(NSETS):
                point = dict(zip(corr.correction_names, coefs[i]))
                disp[i] = corr.get_displacements({}, point=point)
            out["strain%d_los" % b] = lv
            out["strain%d_disp" % b] = disp
    finally:
        heart.orthodrome = real
    out.update({"strain_norths": norths, "strain_easts": easts, "strain_lats": lats, "strain_lons": lons,
                "strain_mask": mask, "strain_coefs": coefs})


def main():
    rng = np.random.default_rng(20261016)
    out = {"note": np.array(
        "ramp: local coordinates are seeded uniform +-30 km [m], not the scenes' own (the pickled scenes hold lons/lats "
        "only); data/odw are the Laquila scenes'; mu is seeded N(0, 0.05). strain: norths/easts [m] are seeded and were "
        "handed to the reference through a replaced heart.orthodrome; lats/lons are placeholders. disp/res come from "
        "the reference's RampCorrection / StrainRateCorrection.get_displacements(point=...).")}
    gen_ramp(out, rng)
    gen_strain(out, rng)
    path = os.path.join(GOLDEN, "geo_corrections.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f kB)" % (path, os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
