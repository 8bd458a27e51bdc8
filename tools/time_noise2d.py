"""Times of one geodetic non-Toeplitz data covariance update (beat_amd.covariance.GeodeticNoiseCovarianceUpdate) on one
MI355X, one process, at two shapes:

    scenes    two SAR scenes of 214 and 205 points (the Laquila sizes), max_dist_perc 0.2
    large     one scene of 4096 points, max_dist_perc 0.1

Legs, alternated round by round:

    device    ``update_weights`` as shipped, between host clocks around device synchronisations
    steps     the same calls one by one with a synchronisation after each: residual (the model's mu, data - mu), ball
              statistic (``beatamd_ball_rms_batch``), autocovariance, scaled Toeplitz, factorisation + installation.  The
              synchronisations make their sum larger than the update.
    host      the estimate composed on the host of the GPU machine: the residual downloaded, scipy's KD-tree and numpy.std
              per point as in the reference's k_nearest_neighbor_rms, numpy's correlation for the autocovariance, the
              scaled Toeplitz matrix, uploaded, then the same device factorisation and installation

    python tools/time_noise2d.py [--out profiles/noise2d_timing.json] [--reps 3]

Each leg: one warm-up call, then ``reps`` rounds; reported: the median of the rounds with min and max.  Nothing gates on
these numbers."""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise2d_timing.json"))
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

import torch  # noqa: E402

import beat_amd  # noqa: E402
from beat_amd.covariance import GeodeticNoiseCovarianceUpdate  # noqa: E402
from beat_amd.ffi import GeodeticGFLibrary, GeodeticGFLibraryConfig  # noqa: E402
from beat_amd.heart import Covariance  # noqa: E402
from beat_amd.models import FFIProblem, GeodeticData, ParameterLayout  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
dev = torch.device("cuda", 0)
SLIPS = ("uparr", "uperp")
STEPS = ("residual", "ball_rms", "autocovariance", "scaled_toeplitz", "factorise_install")


def build(sizes, P, seed):
    rng = np.random.default_rng(seed)
    nobs = sum(sizes)
    gfs = {}
    q = np.zeros(2 * P + 1)
    mu = np.zeros(nobs)
    for iv, v in enumerate(SLIPS):
        gf = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=(P, nobs), component=v))
        gf.setup(P, nobs, allocate=True)
        gf._gfmatrix[:] = 0.02 * rng.standard_normal((P, nobs))
        gfs[v] = gf
        q[iv * P:(iv + 1) * P] = rng.uniform(0.0, 3.0, P)
        mu += np.asarray(gf._gfmatrix).T @ q[iv * P:(iv + 1) * P]
    coords = [rng.uniform(-20e3, 20e3, (n, 2)) for n in sizes]
    covs = [Covariance(data=4e-6 * np.eye(n)) for n in sizes]
    lay = ParameterLayout(OrderedDict([(v, P) for v in SLIPS] + [("h_SAR", 1)]))
    geo = GeodeticData(gfs, mu + 2e-3 * rng.standard_normal(nobs), np.ones(nobs), sizes, [c.chol_inverse for c in covs],
                       [float(c.log_pdet) for c in covs], [("h_SAR", 0)] * len(sizes))
    prob = FFIProblem(lay, [], [], [], SLIPS, geodetic=geo, lower=dict(uparr=0.0, uperp=0.0, h_SAR=-1.0),
                      upper=dict(uparr=3.0, uperp=3.0, h_SAR=1.0))
    return prob.compile(ctx), coords, covs, q


def clocked(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    r = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def install(f, mats):
    Ws, lps = [], []
    for C in mats:
        W, lp, bad = ctx.chol_inverse_batch_flags(C.unsqueeze(0))
        assert not int(bad[0])
        Ws.append(W[0])
        lps.append(float(lp[0]))
    f.update_geodetic_weights(Ws, lps)


def stepwise(f, upd, q, perc, split):
    sizes = list(f.problem.geodetic.sizes)
    t, res = clocked(lambda: upd.residuals(q))
    split["residual"].append(t)
    t, (_, _, stds) = clocked(lambda: ctx.ball_rms_batch(upd._resident()["coords"], res, sizes, perc))
    split["ball_rms"].append(t)
    o, parts = 0, []
    for n in sizes:
        parts.append((res[o:o + n].reshape(1, n), stds[o:o + n].reshape(1, n)))
        o += n
    t, coeffs = clocked(lambda: [ctx.autocovariance_batch(r / s) for r, s in parts])
    split["autocovariance"].append(t)
    t, mats = clocked(lambda: [ctx.scaled_toeplitz_batch(c, s)[0] for c, (_, s) in zip(coeffs, parts)])
    split["scaled_toeplitz"].append(t)
    t, _ = clocked(lambda: install(f, mats))
    split["factorise_install"].append(t)


def host_update(f, upd, q, perc):
    """the estimate with scipy's KD-tree and numpy on the host, then the device factorisation"""
    from scipy.spatial import KDTree
    res = upd.residuals(q).cpu().numpy()
    mats, o = [], 0
    for n, c in zip(f.problem.geodetic.sizes, upd.coords):
        r = res[o:o + n]
        d2 = 0.0
        for a in range(0, n, 512):
            d = c[a:a + 512, None, :] - c[None, :, :]
            d2 = max(d2, float((d * d).sum(axis=2).max()))
        radius = np.sqrt(d2) * perc
        tree = KDTree(c, leafsize=1)
        stds = np.array([np.std(r[tree.query_ball_point(p, r=radius)], ddof=1) for p in c])
        x = r / stds
        x = x - x.mean()
        coeffs = np.correlate(x, x, mode="full")[n - 1:] / n
        i = np.arange(n)
        mats.append(torch.from_numpy(coeffs[np.abs(i[:, None] - i[None, :])] * stds[:, None] * stds[None, :]).to(dev))
        o += n
    install(f, mats)


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), n=len(v))


def leg(sizes, P, perc, seed):
    f, coords, covs, q = build(sizes, P, seed)
    upd = GeodeticNoiseCovarianceUpdate(f, coords, covs, perc)
    split = {k: [] for k in STEPS}
    legs = OrderedDict([("device", lambda: upd.update_weights(q)), ("steps", lambda: stepwise(f, upd, q, perc, split)),
                        ("host", lambda: host_update(f, upd, q, perc))])
    for fn in legs.values():
        fn()
    split = {k: [] for k in STEPS}
    ts = {k: [] for k in legs}
    for _ in range(args.reps):
        for name, fn in legs.items():
            ts[name].append(clocked(fn)[0])
    res = {k: stats(v) for k, v in ts.items() if k != "steps"}
    res["device_by_step"] = {k: stats(v) for k, v in split.items()}
    res["shape"] = dict(sizes=list(sizes), max_dist_perc=perc, nvar=len(SLIPS), P=P,
                        pair_tests=int(sum(3 * n * n for n in sizes)), matrix_bytes=int(sum(n * n * 8 for n in sizes)))
    assert upd.n_host_route == 0
    f.release()
    return res


out = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
       "scenes": leg((214, 205), 400, 0.2, 1), "large": leg((4096,), 400, 0.1, 2)}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
