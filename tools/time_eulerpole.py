"""What one Euler-pole term costs the fused Metropolis step on one MI355X, one process, the two sides alternated:

  laquila_ffi    a 512-chain FFI geodetic model of the Laquila scenes' size (214 + 205 points, full covariances, three
                 slip variables on 240 patches) plus a 72-row GNSS dataset
  config4_N120   BASELINE configs[3] at 120 samples (tools/time_summary.py's leg) with a 72-row GNSS dataset beside its
                 two geodetic scenes, 512 chains

each `without` (the 72-row dataset carries no correction: the code path of a pole-free table, no k_pole_coef launch)
and `with` one pole term on that dataset (pole_lat, pole_lon, omega sampled).  The three pole variables are part of
the parameter vector on both sides, so the proposal costs the same; what differs is one small launch per model
evaluation (k_pole_coef) and three products per row of the 72-row dataset.

    python tools/time_eulerpole.py [--out profiles/eulerpole_timing.json] [--reps 3] [--iters 100]

Each leg: warm-up, then ``reps`` rounds in which the two sides are timed one after the other (``iters`` steps of an SMC
stage between two device events each); reported: the median of the rounds with min and max.  Nothing gates on these
numbers."""
import argparse
import json
import os
import sys
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eulerpole_timing.json"))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--chains", type=int, default=512)
args = ap.parse_args()

import torch  # noqa: E402

import beat_amd  # noqa: E402
from beat_amd.ffi import GeodeticGFLibrary, GeodeticGFLibraryConfig  # noqa: E402
from beat_amd.heart import whitening  # noqa: E402
from beat_amd.models import (EulerPoleConfig, FFIProblem, GeodeticData,  # noqa: E402
                             ParameterLayout)
from beat_amd.sampler import SMC  # noqa: E402
from beat_amd.synthetic import SyntheticSpec, build_problem  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
dev = torch.device("cuda", 0)
NGNSS = 72
POLE_BOUNDS = (("pole_lat", 90.0), ("pole_lon", 180.0), ("omega", 10.0))


def pole_term(rng, number):
    nsta = NGNSS // 3
    lats, lons = np.repeat(rng.uniform(40.0, 44.0, nsta), 3), np.repeat(rng.uniform(11.0, 15.0, nsta), 3)
    c = EulerPoleConfig(dataset_names=["gnss"], enabled=True).init_correction()
    c.setup_correction(lats, lons, np.tile(np.eye(3), (nsta, 1)), np.zeros(NGNSS, dtype=bool), "gnss", number=number)
    lower = dict(("%d_%s" % (number, s), -b) for s, b in POLE_BOUNDS)
    upper = dict(("%d_%s" % (number, s), b) for s, b in POLE_BOUNDS)
    return c, lower, upper


def stage(f, lo, up):
    step = SMC(f, lo, up, n_chains=args.chains, tune_interval=10, device=dev, random_seed=2)
    Q = step.initialize_population()
    L = step.stepper.evaluate(Q)
    step.select_end_points(Q, L)
    step.transition()
    step.stage += 1
    return step


def timed(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    step.sample_stage(iters)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def alternate(steps):
    """steps: side -> SMC object in a stage; -> side -> dict(median_us, min_us, max_us, n) per Metropolis step"""
    for s in steps.values():
        s.sample_stage(max(args.iters // 4, 5))
    torch.cuda.synchronize()
    ts = {k: [] for k in steps}
    for _ in range(args.reps):
        for k, s in steps.items():
            ts[k].append(timed(s, args.iters))
    out = {k: dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)), n=len(v))
           for k, v in ts.items()}
    out["pole_term_us"] = out["with"]["median_us"] - out["without"]["median_us"]
    out["spread_without_us"] = out["without"]["max_us"] - out["without"]["min_us"]
    return out


def laquila_ffi():
    g = np.load(os.path.join(ROOT, "tests", "golden", "laquila_geodetic.npz"))
    rng = np.random.default_rng(7)
    slips, P = ("uparr", "uperp", "utens"), 240
    sizes = [int(g["d%d_displacement" % d].size) for d in range(2)] + [NGNSS]
    nobs = sum(sizes)
    gfs = {}
    for v in slips:
        gg = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=(P, nobs), component=v))
        gg.setup(P, nobs, allocate=True)
        gg._gfmatrix[:] = 1e-2 * rng.standard_normal((P, nobs))
        gfs[v] = gg
    Ws, sls = zip(*([whitening(g["d%d_C" % d]) for d in range(2)] + [whitening(1e-6 * np.eye(NGNSS))]))
    data = np.concatenate([g["d%d_displacement" % d] for d in range(2)] + [1e-2 * rng.standard_normal(NGNSS)])
    odw = np.concatenate([g["d%d_odw" % d] for d in range(2)] + [np.ones(NGNSS)])
    pole, plo, pup = pole_term(rng, 2)
    lay = ParameterLayout(OrderedDict([(v, P) for v in slips] + [(n, 1) for n in pole.correction_names] + [("h_SAR", 1)]))
    lower = dict(dict((v, -0.05) for v in slips), h_SAR=-1.0, **plo)
    upper = dict(dict((v, 0.05) for v in slips), h_SAR=1.0, **pup)
    lo, up = lay.bounds(lower, upper)
    steps = {}
    for side, corrs in (("without", None), ("with", [[], [], [pole]])):
        geo = GeodeticData(gfs, data, odw, sizes, list(Ws), list(sls), [("h_SAR", 0)] * 3, corrections=corrs)
        steps[side] = stage(FFIProblem(lay, [], [], [], slips, geodetic=geo, lower=lower, upper=upper).compile(ctx), lo, up)
    res = alternate(steps)
    res["shape"] = dict(chains=args.chains, patches=P, slip_variables=3, geodetic_nobs=sizes)
    return res


def config4_n120():
    spec = SyntheticSpec((10, 10), (20, 20), (2.0, 2.0), T=35, N=120, D=2, S=60, st_dt=0.5,
                         slip_varnames=("uparr", "uperp"), covariance="toeplitz", station_shifts=True,
                         geodetic_nobs=(214, 214, NGNSS), vel_bounds=(3.0, 4.0), time_bounds=(0.0, 2.0))
    pole, plo, pup = pole_term(np.random.default_rng(11), 2)
    steps = {}
    for side in ("without", "with"):
        prob, host = build_problem(spec, device_library=True, ctx=ctx)
        lay = ParameterLayout(OrderedDict(list(host["layout"].varsizes.items()) + [(n, 1) for n in pole.correction_names]))
        prob.layout = lay
        lo, up = lay.bounds(dict(host["lower"], **plo), dict(host["upper"], **pup))
        if side == "with":
            prob.geodetic.corrections = [[], [], [pole]]
        steps[side] = stage(prob.compile(ctx), lo, up)
    res = alternate(steps)
    res["shape"] = dict(chains=args.chains, T=spec.T, N=spec.N, P=spec.P, D=spec.D, S=spec.S,
                        covariance=spec.covariance, geodetic_nobs=list(spec.geodetic_nobs))
    return res


out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters,
       "what": "microseconds per fused Metropolis step of an SMC stage; median of the rounds, min and max",
       "laquila_ffi": laquila_ffi(), "config4_N120": config4_n120()}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
