"""Times of one velocity-model prediction covariance update (beat_amd.covariance.VelocityModelCovarianceUpdate) on one
MI355X, one process, at two shapes:

    scenes    two datasets of 214 and 205 points, K = 12 crust variants, two slip variables of 400 patches
    large     one dataset of 4096 points, K = 40 variants, two slip variables of 400 patches

Two legs, alternated round by round:

    device    ``update_weights`` as shipped: ensemble stack, sample covariance onto the resident data covariance,
              factorisation, installation -- with the library's event timers on, so the update is split by kernel
              (cruststack, predcenter, predcov, chol_inverse)
    host      the same update composed on the host of the GPU machine: the stack downloaded, ``numpy.cov`` per dataset plus
              the data covariance, the totals uploaded, then the same device factorisation and installation

    python tools/time_predcov.py [--out profiles/predcov_timing.json] [--reps 3]

Each leg: one warm-up call, then ``reps`` rounds, one call per leg and round between host clocks around device
synchronisations; reported: the median of the rounds with min and max.  Nothing gates on these numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predcov_timing.json"))
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

import torch  # noqa: E402

import beat_amd  # noqa: E402
from beat_amd.covariance import VelocityModelCovarianceUpdate  # noqa: E402
from beat_amd.ffi import GeodeticGFEnsemble, GeodeticGFLibrary, GeodeticGFLibraryConfig  # noqa: E402
from beat_amd.heart import Covariance  # noqa: E402
from beat_amd.models import FFIProblem, GeodeticData, ParameterLayout  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
dev = torch.device("cuda", 0)
SLIPS = ("uparr", "uperp")
KERNELS = ("cruststack", "predcenter", "predcov", "chol_inverse")


def build(sizes, K, P, seed):
    from collections import OrderedDict
    rng = np.random.default_rng(seed)
    nobs = sum(sizes)
    G0 = 0.02 * rng.standard_normal((len(SLIPS), P, nobs))
    libs = {}
    for k in range(K):
        libs[k] = {}
        for iv, v in enumerate(SLIPS):
            gf = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=(P, nobs), component=v, crust_ind=k))
            gf.setup(P, nobs, allocate=True)
            gf._gfmatrix[:] = G0[iv] if k == 0 else G0[iv] * (1.0 + 0.02 * rng.standard_normal((P, nobs)))
            libs[k][v] = gf
    ens = GeodeticGFEnsemble(libs, SLIPS)
    covs = []
    for n in sizes:
        i = np.arange(n)
        covs.append(Covariance(data=1e-5 * (np.exp(-np.abs(i[:, None] - i[None, :]) / 5.0) + 0.1 * np.eye(n))))
    lay = ParameterLayout(OrderedDict([(v, P) for v in SLIPS] + [("h_SAR", 1)]))
    geo = GeodeticData(libs[0], 0.05 * rng.standard_normal(nobs), np.ones(nobs), sizes, [c.chol_inverse for c in covs],
                       [float(c.log_pdet) for c in covs], [("h_SAR", 0)] * len(sizes))
    prob = FFIProblem(lay, [], [], [], SLIPS, geodetic=geo, lower=dict(uparr=0.0, uperp=0.0, h_SAR=-1.0),
                      upper=dict(uparr=3.0, uperp=3.0, h_SAR=1.0))
    q = np.concatenate([rng.uniform(0.0, 3.0, 2 * P), [0.0]])
    return prob.compile(ctx), ens, covs, q


def host_update(f, upd, q):
    """the update with the sample covariance formed by numpy on the host"""
    X = upd.crust_synthetics(q).cpu().numpy()
    Ws, lps, o = [], [], 0
    for n, cov in zip(f.problem.geodetic.sizes, upd.covariances):
        total = cov.data + np.atleast_2d(np.cov(X[:, o:o + n], rowvar=0))
        W, lp, bad = ctx.chol_inverse_batch_flags(torch.from_numpy(total[None]).to(dev))
        assert not int(bad[0])
        Ws.append(W[0])
        lps.append(float(lp[0]))
        o += n
    f.update_geodetic_weights(Ws, lps)
    ctx.synchronize()


def clocked(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), n=len(v))


def leg(sizes, K, P, seed):
    f, ens, covs, q = build(sizes, K, P, seed)
    upd = VelocityModelCovarianceUpdate(f, ens, covs)
    legs = {"device": lambda: upd.update_weights(q), "host": lambda: host_update(f, upd, q)}
    for fn in legs.values():
        fn()
    ts = {k: [] for k in legs}
    kern = {k: [] for k in KERNELS}
    for _ in range(args.reps):
        for name, fn in legs.items():
            if name == "device":
                ctx.enable_timing(True)
                ctx.reset_timing()
            ts[name].append(clocked(fn))
            if name == "device":
                for k in KERNELS:
                    kern[k].append(ctx.kernel_time(k)[0])
                ctx.enable_timing(False)
    res = {k: stats(v) for k, v in ts.items()}
    res["device_by_kernel"] = {k: stats(v) for k, v in kern.items()}
    res["host_over_device"] = res["host"]["median_ms"] / res["device"]["median_ms"]
    nobs = sum(sizes)
    res["shape"] = dict(sizes=list(sizes), K=K, nvar=len(SLIPS), P=P,
                        library_bytes_streamed=K * len(SLIPS) * P * nobs * 8,
                        matrix_bytes=int(sum(2 * n * n * 8 for n in sizes)))
    assert upd.n_host_route == 0
    f.release()
    ens.release()
    return res


out = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
       "scenes": leg((214, 205), 12, 400, 1), "large": leg((4096,), 40, 400, 2)}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
