"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/pred_cov.npz by running the REFERENCE's own code on seeded inputs: the velocity-model prediction
covariance of the geodetic datasets as GeodeticDistributerComposite.update_weights forms it.  Needs the reference tree
(oracle/ref_import.py finds it), so it runs where that tree is mounted; the fixture it writes is data (inputs and
expected outputs, none of the reference's text).

    python tools/gen_golden_predcov.py

Reference entry points exercised:
  beat/ffi/base.py:292-305          GeodeticGFLibrary.stack_all (numpy mode), per crust variant and slip variable,
                                    summed as beat/models/geodetic.py:1167-1176 sums them
  beat/models/geodetic.py:1187      num.cov(crust_synths[i], rowvar=0)
  beat/utility.py:1034-1056, 1111-1138   ensure_cov_psd / repair_covariance
  beat/heart.py:104-253             Covariance(data=..., pred_v=...).chol_inverse / .log_pdet

Two cases.
  small    K = 7 variants, nvar = 2, P = 5, datasets of 1, 30 and 33 points with seeded SPD data covariances.  Everything is
           stored: libraries, slips, X, raw and repaired cov_pv, W, log_pdet.  num.cov of ONE column is a 0-d array, which
           ensure_cov_psd cannot take (cholesky and eigh both refuse it): the one-point dataset's value is handed on as a
           (1, 1) matrix.
  laquila  the two scenes of tests/golden/laquila_geodetic.npz (214 and 205 points, their C), K = 7, nvar = 2, P = 6:
           libraries, slips, X, log_pdet of the total, and |W r|^2 for four stored residual vectors per scene.  The
           operators and cov_pv are not stored (they would be the largest fixture; a test rebuilds them from X).
Library values: a seeded reference library G_0 ~ 0.02 N(0, 1) [m per m of slip] and variants G_k = G_0 (1 + 0.02 N(0, 1)):
millimetres of spread between the variants' synthetics, the size of the scenes' data errors.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402

ref_import.install()

from beat import heart, utility  # noqa: E402
from beat.config import GeodeticGFLibraryConfig  # noqa: E402
from beat.ffi import base as ffibase  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
K, NVAR = 7, 2


def libraries(rng, P, nobs):
    """[K, NVAR, P, nobs]"""
    G0 = 0.02 * rng.standard_normal((NVAR, P, nobs))
    G = np.stack([G0 * (1.0 + 0.02 * rng.standard_normal(G0.shape)) for _ in range(K)])
    G[0] = G0
    return G


def crust_synthetics(G, slips):
    """geodetic.py:1167-1176 with the reference's library objects in numpy mode"""
    nvar, P, nobs = G.shape[1:]
    X = np.zeros((G.shape[0], nobs))
    for k in range(G.shape[0]):
        mu = np.zeros(nobs)
        for v in range(nvar):
            gf = ffibase.GeodeticGFLibrary(config=GeodeticGFLibraryConfig(dimensions=(P, nobs)))
            gf.setup(P, nobs, allocate=True)
            gf._gfmatrix[:] = G[k, v]
            gf._stack_switch = {"numpy": gf._gfmatrix}
            mu += gf.stack_all(slips=slips[v])
        X[k, :] = mu
    return X


def pred_v(X):
    """geodetic.py:1187-1189 -> (raw, repaired)"""
    raw = np.atleast_2d(np.cov(X, rowvar=0))
    return raw, utility.ensure_cov_psd(raw)


def gen_small(out, rng):
    sizes = [1, 30, 33]
    P, nobs = 5, sum(sizes)
    G = libraries(rng, P, nobs)
    slips = rng.uniform(0.0, 3.0, (NVAR, P))
    X = crust_synthetics(G, slips)
    out.update(small_G=G, small_slips=slips, small_X=X, small_sizes=np.array(sizes))
    o = 0
    for i, n in enumerate(sizes):
        b = rng.standard_normal((n, n))
        Cd = 1e-5 * (b @ b.T / n + np.eye(n))
        raw, rep = pred_v(X[:, o:o + n])
        cov = heart.Covariance(data=Cd, pred_v=rep)
        out.update({"small_C%d" % i: Cd, "small_raw%d" % i: raw, "small_rep%d" % i: rep,
                    "small_W%d" % i: cov.chol_inverse, "small_logpdet%d" % i: np.array(cov.log_pdet)})
        o += n


def gen_laquila(out, rng):
    laq = np.load(os.path.join(GOLDEN, "laquila_geodetic.npz"))
    nd = int(laq["n"])
    sizes = [int(laq["d%d_displacement" % d].size) for d in range(nd)]
    P, nobs = 6, sum(sizes)
    G = libraries(rng, P, nobs)
    slips = rng.uniform(0.0, 3.0, (NVAR, P))
    X = crust_synthetics(G, slips)
    out.update(laquila_G=G, laquila_slips=slips, laquila_X=X, laquila_sizes=np.array(sizes))
    o = 0
    for d, n in enumerate(sizes):
        raw, rep = pred_v(X[:, o:o + n])
        cov = heart.Covariance(data=laq["d%d_C" % d], pred_v=rep)
        W = cov.chol_inverse
        # residuals of the scene against the first four variants' synthetics, with the scene's odw factor
        r = (laq["d%d_displacement" % d][None, :] - X[:4, o:o + n]) * laq["d%d_odw" % d][None, :]
        out.update({"laquila_logpdet%d" % d: np.array(cov.log_pdet), "laquila_r%d" % d: r,
                    "laquila_quad%d" % d: np.array([W.dot(x).dot(W.dot(x)) for x in r]),
                    "laquila_repair_shift%d" % d: np.array(np.abs(rep - raw).max())})
        o += n


def main():
    rng = np.random.default_rng(20261019)
    out = {"note": np.array(
        "X = the reference's GeodeticGFLibrary.stack_all (numpy mode) summed over the slip variables per crust variant; "
        "raw = num.cov(X[:, dataset], rowvar=0) (a one-point dataset's 0-d value as a (1, 1) matrix); rep = "
        "utility.ensure_cov_psd(raw); W / logpdet = heart.Covariance(data=C, pred_v=rep).chol_inverse / .log_pdet; "
        "laquila: C = d<i>_C of laquila_geodetic.npz, quad = |W r|^2 of the stored residual vectors.")}
    gen_small(out, rng)
    gen_laquila(out, rng)
    path = os.path.join(GOLDEN, "pred_cov.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f kB)" % (path, os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
