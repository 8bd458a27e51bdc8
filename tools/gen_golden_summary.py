"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/summary.npz by running the REFERENCE's own covariance arithmetic on seeded inputs.  Needs the
reference tree (oracle/ref_import.py finds it), so it runs where that tree is mounted; the fixture it writes is data
(inputs and expected outputs, none of the reference's text).

    python tools/gen_golden_summary.py

Reference entry points exercised:
  beat/heart.py:104-263               Covariance(data=..., pred_v=...): chol_inverse, inverse(factor), chol(factor)
  beat/models/seismic.py:610-620      the numpy lines of get_variance_reductions: icov = inverse(exp(hp * 2)),
                                      nom = r.T.dot(icov).dot(r), denom = d.T.dot(icov).dot(d), 1 - nom / denom
  beat/models/seismic.py:560-561      the numpy lines of get_standardized_residuals:
                                      inv(covariance.chol(exp(hp * 2))).dot(r)
  beat/plotting/seismic.py:400-402    floor(arange(0, nchains, float(nchains) / nensemble)).astype("int32")

get_variance_reductions / get_standardized_residuals themselves need a whole project (datasets, targets, a forward
model); their numpy lines are applied here to seeded vectors through the reference's own Covariance object.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402

ref_import.install()

from beat import heart  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

SIZES = (1, 8, 33, 64)
KINDS = ("scalar", "toeplitz", "toeplitz_predv", "spd")
HPS = (0.0, 1.7, -2.3)
ENSEMBLES = ((10, 4), (530, 7), (5, 5), (3, 5), (4096, 100))
# inverse(exp(2 hp)) and chol(exp(2 hp)) are six more n x n matrices per case: kept for n <= 8, where they fit the
# 200 kB the fixture may take; at n = 33 and 64 what the reference derives from them (nom, denom, vr, z) is kept
FULL_MATRICES_UP_TO = 8


def _covariance(kind, n, rng):
    """-> (data, pred_v or None)"""
    i = np.arange(n)
    toeplitz = np.exp(-np.abs(i[:, None] - i[None, :]) * (0.5 / 2.0))        # the "exponential" structure, dt / tzero
    if kind == "scalar":
        return rng.uniform(0.5, 2.0) ** 2 * np.eye(n), None
    if kind == "toeplitz":
        return rng.uniform(0.5, 2.0) ** 2 * toeplitz, None
    if kind == "toeplitz_predv":
        return toeplitz, np.diag(rng.uniform(0.05, 0.5, n))
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))                          # eigenvalues over four decades at most
    ev = 10.0 ** rng.uniform(-2.0, 2.0, n)
    C = (q * ev) @ q.T
    return 0.5 * (C + C.T), None


def main():
    rng = np.random.default_rng(20261018)
    out = {"note": np.array(
        "<kind>_<n>_*: data / pred_v handed to the reference's heart.Covariance; chol_inverse its property; d, r seeded; "
        "per hp in `hps`: inverse_<i> = inverse(exp(2 hp)), chol_<i> = chol(exp(2 hp)) (n <= 8 only), nom/denom/vr the numpy lines of "
        "seismic.py:610-620, z_<i> those of seismic.py:560-561. ens_<n>_<e>: the raw output of the reference's "
        "ensemble-index expression (plotting/seismic.py:400-402), overshoot included."),
        "sizes": np.asarray(SIZES), "kinds": np.array(KINDS), "hps": np.asarray(HPS)}
    for kind in KINDS:
        for n in SIZES:
            data, pred_v = _covariance(kind, n, rng)
            cov = heart.Covariance(data=data, pred_v=pred_v) if pred_v is not None else heart.Covariance(data=data)
            d = 3.0 * rng.standard_normal(n)
            r = rng.standard_normal(n)
            k = "%s_%d" % (kind, n)
            out[k + "_data"] = data
            if pred_v is not None:
                out[k + "_pred_v"] = pred_v
            out[k + "_chol_inverse"] = np.asarray(cov.chol_inverse)
            out[k + "_d"], out[k + "_r"] = d, r
            nom, denom, vr = [], [], []
            for i, hp in enumerate(HPS):
                icov = cov.inverse(np.exp(hp * 2.0))
                if n <= FULL_MATRICES_UP_TO:
                    out[k + "_inverse_%d" % i] = np.asarray(icov)
                    out[k + "_chol_%d" % i] = np.asarray(cov.chol(np.exp(hp * 2.0)))
                nom.append(r.T.dot(icov).dot(r))
                denom.append(d.T.dot(icov).dot(d))
                vr.append(float(1 - (nom[-1] / denom[-1])))
                choli = np.linalg.inv(cov.chol(np.exp(hp * 2.0)))
                out[k + "_z_%d" % i] = choli.dot(r)
            out[k + "_nom"], out[k + "_denom"], out[k + "_vr"] = np.asarray(nom), np.asarray(denom), np.asarray(vr)
    for nchains, nensemble in ENSEMBLES:
        csteps = float(nchains) / nensemble
        out["ens_%d_%d" % (nchains, nensemble)] = np.floor(np.arange(0, nchains, csteps)).astype("int32")
    out["ens_cases"] = np.asarray(ENSEMBLES, dtype=np.int64)
    path = os.path.join(GOLDEN, "summary.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f kB)" % (path, os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
