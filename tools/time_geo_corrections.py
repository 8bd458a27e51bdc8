"""HIP-event times of the two geodetic residual paths with and without dataset corrections:

  (a) geometry  the 1024-chain geometry step of tools/geo_app.py's shape (one rectangular source, two scenes of
                214 + 205 points, full covariances): the batched likelihood (k_geom_los + k_quadform_small) and the
                Metropolis step of an SMC stage
  (b) ffi       a 512-chain FFI evaluation on the Laquila scenes (three slip variables): k_geo_stack + k_geo_residual +
                the dense quadratic forms

    python tools/time_geo_corrections.py [--corrections none|ramps] [--root DIR] [--reps 7] [--iters 200] [--short]

--corrections none uses nothing but the interface of a tree without the feature, so the same script times the
parent commit: --root DIR imports beat_amd from a checkout of it (alternate the two builds process by process and
compare the medians with the spread the parent shows by itself).  --short: few iterations, for a
`rocprofv3 --kernel-trace --stats` run (kernel names and dispatch counts of the two builds).
Prints one JSON line."""
import argparse
import json
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--corrections", choices=("none", "ramps"), default="none")
ap.add_argument("--root", default=HERE)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--short", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402

import beat_amd  # noqa: E402
from beat_amd.ffi import GeodeticGFLibrary, GeodeticGFLibraryConfig  # noqa: E402
from beat_amd.heart import whitening  # noqa: E402
from beat_amd.models import (FFIProblem, GeodeticData, GeodeticGeometryProblem,  # noqa: E402
                             ParameterLayout)
from beat_amd.sampler import SMC  # noqa: E402
from beat_amd.synthetic import build_geometry_problem  # noqa: E402

RAMPS = args.corrections == "ramps"
if args.short:
    args.reps, args.iters = 1, 20
ctx = beat_amd.get_context(0)
dev = torch.device("cuda", 0)
SUFFIX_BOUNDS = (("azimuth_ramp", 0.1), ("range_ramp", 0.1), ("offset", 0.05))


def ramps(norths, easts):
    """one ramp per scene (coordinates in metres) -> corrections, variable names, bounds"""
    from beat_amd.models import RampConfig
    names = ["scene_%d" % d for d in range(len(norths))]
    cfg = RampConfig(dataset_names=names, enabled=True)
    corrs, lower, upper = [], {}, {}
    for name, n, e in zip(names, norths, easts):
        c = cfg.init_correction()
        c.setup_correction(n, e, None, None, name)
        corrs.append([c])
        for v, (_, b) in zip(c.correction_names, SUFFIX_BOUNDS):
            lower[v], upper[v] = -b, b
    return corrs, list(lower), lower, upper


def event_times(fn, reps, iters):
    """reps measurements of `iters` back-to-back calls between two events -> microseconds per call"""
    for _ in range(max(iters // 4, 5)):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters * 1e3)
    return out


def summary(ts):
    return dict(median_us=float(np.median(ts)), min_us=float(np.min(ts)), max_us=float(np.max(ts)), n=len(ts))


def geometry():
    prob, lay, lower, upper = build_geometry_problem()
    if RAMPS:
        o, ns, es = 0, [], []
        for n in prob.sizes:
            ns.append(prob.north[o:o + n] * 1e3)
            es.append(prob.east[o:o + n] * 1e3)
            o += n
        corrs, cnames, clo, cup = ramps(ns, es)
        lay = ParameterLayout(OrderedDict(list(lay.varsizes.items()) + [(n, 1) for n in cnames]))
        lower, upper = dict(lower, **clo), dict(upper, **cup)
        prob = GeodeticGeometryProblem(lay, prob.sources, prob.east, prob.north, prob.los, prob.data, prob.odws,
                                       prob.sizes, prob.weights, prob.slog_pdets, prob.hypers, fixed=prob.fixed,
                                       lower=lower, upper=upper, corrections=corrs)
    lo, up = lay.bounds(lower, upper)
    f = prob.compile(ctx)
    C = 1024
    step = SMC(f, lo, up, n_chains=C, tune_interval=10, device=dev, random_seed=2)
    Q = step.initialize_population()
    L = step.stepper.evaluate(Q)
    step.select_end_points(Q, L)
    step.transition()
    step.stage += 1
    Qd = Q.contiguous()
    out = torch.empty((C, f.nllk), dtype=torch.float64, device=dev)
    res = {"logp_1024": summary(event_times(lambda: f.batch(Qd, out), args.reps, args.iters))}
    ts = []
    step.sample_stage(max(args.iters // 4, 5))
    torch.cuda.synchronize()
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step.sample_stage(args.iters)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / args.iters * 1e3)
    res["metropolis_step_1024"] = summary(ts)
    return res


def ffi():
    g = np.load(os.path.join(HERE, "tests", "golden", "laquila_geodetic.npz"))
    rng = np.random.default_rng(7)
    slips, P = ("uparr", "uperp", "utens"), 240
    sizes = [int(g["d%d_displacement" % d].size) for d in range(2)]
    nobs = sum(sizes)
    gfs = {}
    for v in slips:
        gg = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=(P, nobs), component=v))
        gg.setup(P, nobs, allocate=True)
        gg._gfmatrix[:] = 1e-2 * rng.standard_normal((P, nobs))
        gfs[v] = gg
    Ws, sls = zip(*[whitening(g["d%d_C" % d]) for d in range(2)])
    data = np.concatenate([g["d%d_displacement" % d] for d in range(2)])
    odw = np.concatenate([g["d%d_odw" % d] for d in range(2)])
    names = [(v, P) for v in slips]
    kw = {}
    if RAMPS:
        corrs, cnames, _, _ = ramps([rng.uniform(-30e3, 30e3, n) for n in sizes],
                                    [rng.uniform(-30e3, 30e3, n) for n in sizes])
        names += [(n, 1) for n in cnames]
        kw = dict(corrections=corrs)
    lay = ParameterLayout(OrderedDict(names + [("h_SAR", 1)]))
    geo = GeodeticData(gfs, data, odw, sizes, list(Ws), list(sls), [("h_SAR", 0)] * 2, **kw)
    f = FFIProblem(lay, [], [], [], slips, geodetic=geo).compile(ctx)
    C = 512
    Q = torch.from_numpy(rng.uniform(-0.05, 0.05, (C, lay.size))).to(dev)
    out = torch.empty((C, f.nllk), dtype=torch.float64, device=dev)
    return {"logp_512": summary(event_times(lambda: f.batch(Q, out), args.reps, args.iters))}


print(json.dumps({"corrections": args.corrections, "root": os.path.abspath(args.root), "iters": args.iters,
                  "geometry": geometry(), "ffi": ffi()}))
