"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/noise2d.npz by running the REFERENCE's own code on seeded inputs: the "non-toeplitz" data covariance
of a geodetic scene as GeodeticNoiseAnalyser.do_non_toeplitz forms it from the residual at a point.  Needs the reference
tree (oracle/ref_import.py finds it), so it runs where that tree is mounted; the fixture it writes is data (inputs and
expected outputs, none of the reference's text).

    python tools/gen_golden_noise2d.py

Reference entry points exercised:
  beat/covariance.py:774-811        k_nearest_neighbor_rms (max_dist_perc branch; scipy's KDTree, numpy.std(ddof=1))
  beat/utility.py distances         the radius' largest point distance
  beat/covariance.py:716-736        autocovariance of residual / stds
  beat/covariance.py:831-848        non_toeplitz_covariance_2d (asserted equal to toeplitz(coeffs) * stds stds^T)
  beat/heart.py:104-253             Covariance(data=C_d).log_pdet

Vectors are stored, not matrices: per case coords, residuals, max_dist_perc, radius, the KD-tree's neighbour counts, stds,
coeffs and log_pdet; C_d = toeplitz(coeffs) * stds stds^T is rebuilt by the tests.  Cases (seeded uniform coordinates in
+-20 km, residuals ~ 2 mm N(0, 1)):
  n30, n33   at max_dist_perc 0.4
  laq0, laq1 the two Laquila scene sizes (214, 205) at 0.2, the second with a 50 mm mean offset
  n1024      at 0.1
  grid       the 4 x 5 unit grid at 0.2: the largest distance is 5, the radius exactly 1.0, every neighbour a tie
  lone       n = 30 at 0.2, one point moved away from all others: counts and the NaN position only
The generator asserts that C_d of every non-NaN case is positive definite without repair, that its condition number is
below 1e3 and that every point has at least 3 neighbours, and reports the numbers.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402

ref_import.install()

from scipy.linalg import toeplitz  # noqa: E402
from scipy.spatial import KDTree  # noqa: E402

from beat import covariance as rcov  # noqa: E402
from beat import heart, utility  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("n30", "n33", "laq0", "laq1", "n1024", "grid", "lone")


def kd_counts(coords, perc):
    """the neighbour sets' sizes, as k_nearest_neighbor_rms obtains the sets (covariance.py:793-805)"""
    tree = KDTree(coords, leafsize=1)
    r = utility.distances(coords, coords).max() * perc
    return r, np.array([len(tree.query_ball_point(p, r=r)) for p in coords], dtype=np.int32)


def scene(rng, n, offset=0.0):
    return rng.uniform(-20e3, 20e3, (n, 2)), offset + 2e-3 * rng.standard_normal(n)


def gen_case(out, name, coords, res, perc, full=True):
    radius, counts = kd_counts(coords, perc)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # numpy.std of one value (the lone point)
        stds = rcov.k_nearest_neighbor_rms(coords, res, max_dist_perc=perc)
    out.update({name + "_coords": coords, name + "_res": res, name + "_perc": np.array(perc),
                name + "_radius": np.array(radius), name + "_counts": counts})
    if not full:
        out[name + "_nan"] = np.isnan(stds)
        return
    assert np.isfinite(stds).all() and (stds > 0).all(), name
    coeffs = rcov.autocovariance(res / stds)
    Cd = rcov.non_toeplitz_covariance_2d(coords, res, max_dist_perc=perc)
    assert np.array_equal(Cd, toeplitz(coeffs) * stds[:, None] * stds[None, :]), name
    np.linalg.cholesky(Cd)                                  # positive definite without repair
    assert np.array_equal(utility.ensure_cov_psd(Cd), Cd), name
    assert counts.min() >= 3 and np.linalg.cond(Cd) < 1e3, name
    cov = heart.Covariance(data=Cd)
    out.update({name + "_stds": stds, name + "_coeffs": coeffs, name + "_logpdet": np.array(cov.log_pdet)})
    print("%-6s n = %4d  radius %.6g  neighbours %d..%d  cond(C_d) %.3g  log_pdet %.6f"
          % (name, res.size, radius, counts.min(), counts.max(), np.linalg.cond(Cd), cov.log_pdet))


def main():
    rng = np.random.default_rng(20261020)
    out = {"note": np.array(
        "per case: coords (n, 2) east / north [m], res (n,) [m], perc = max_dist_perc; radius = utility.distances(coords, "
        "coords).max() * perc; counts = len(KDTree(coords, leafsize=1).query_ball_point(point, r=radius)) per point; stds = "
        "covariance.k_nearest_neighbor_rms; coeffs = covariance.autocovariance(res / stds); logpdet = heart.Covariance("
        "data=C_d).log_pdet with C_d = covariance.non_toeplitz_covariance_2d = toeplitz(coeffs) * stds stds^T (asserted).  "
        "lone: counts and the NaN mask of stds only."),
        "cases": np.array(CASES)}
    gen_case(out, "n30", *scene(rng, 30), 0.4)
    gen_case(out, "n33", *scene(rng, 33), 0.4)
    gen_case(out, "laq0", *scene(rng, 214), 0.2)
    gen_case(out, "laq1", *scene(rng, 205, offset=50e-3), 0.2)
    gen_case(out, "n1024", *scene(rng, 1024), 0.1)
    gy, gx = np.meshgrid(np.arange(4.0), np.arange(5.0), indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel()], axis=1)
    gen_case(out, "grid", grid, 2e-3 * rng.standard_normal(20), 0.2)
    assert float(out["grid_radius"]) == 1.0
    coords, res = scene(rng, 30)
    coords[:, 0] = 0.25 * coords[:, 0] - 15e3        # 29 points in a 10 km strip in the west,
    coords[17] = (20e3, 0.0)                          # one alone in the east: more than a fifth of the extent from all
    gen_case(out, "lone", coords, res, 0.2, full=False)
    assert int(out["lone_counts"][17]) == 1 and (np.delete(out["lone_counts"], 17) >= 2).all()
    assert np.array_equal(np.nonzero(out["lone_nan"])[0], [17])
    path = os.path.join(GOLDEN, "noise2d.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f kB)" % (path, os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
