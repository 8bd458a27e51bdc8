"""Times of the posterior diagnostics on one MI355X, one process, legs alternated:

  (a) ``variance_reductions`` against ``update_llks`` (the same forward model and misfit kernels; what the variance
      reduction adds is one small kernel and, once, the denominators) for 512 draws on
        config3      BASELINE configs[2], the shape of bench.py's default run: 400 patches, 64 targets x 4096 samples,
                     D = 3, S = 25, scalar covariance, the 62.9 GB library generated in HBM
        config4_N120 BASELINE configs[3] at 120 samples: 2 subfaults x (10 x 20) patches, 35 targets, two slip
                     components, station time shifts, Toeplitz covariance, two geodetic scenes of 214 points
  (b) ``k_ensemble_moments`` against a device-to-device copy of the same C * M * 8 bytes, C = 512 rows of
      M = 64 * 4096 columns

    python tools/time_summary.py [--out profiles/summary_timing.json] [--reps 3] [--iters 10] [--skip-config3]

Each leg: warm-up, then ``reps`` rounds in which the two sides are timed one after the other (``iters`` calls between
two device events each); reported: the median of the rounds with min and max.  Nothing gates on these numbers."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_timing.json"))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--skip-config3", action="store_true", help="leave out the 62.9 GB library")
args = ap.parse_args()

import torch  # noqa: E402

import beat_amd  # noqa: E402
from beat_amd.synthetic import SyntheticSpec, build_problem, draw_population  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
ctx.use_torch_stream()
dev = torch.device("cuda", 0)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(legs, reps, iters):
    """legs: name -> callable; -> name -> dict(median_ms, min_ms, max_ms, n)"""
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ts[k].append(timed(fn, iters))
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), n=len(v))
            for k, v in ts.items()}


def vr_leg(spec, C=512):
    prob, host = build_problem(spec, device_library=True, ctx=ctx)
    f = prob.compile(ctx)
    Q = torch.from_numpy(draw_population(spec, host["layout"], host["lower"], host["upper"], C)).to(dev)
    llks = torch.empty((C, f.nterm), dtype=torch.float64, device=dev)
    vr = torch.empty((C, f.ndata), dtype=torch.float64, device=dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f.obs_quads()                      # the denominators: computed once, cached on the model
    b.record()
    b.synchronize()
    res = alternate({"update_llks": lambda: f.update_llks(Q, llks),
                     "variance_reductions": lambda: f.variance_reductions(Q, vr)}, args.reps, args.iters)
    ctx.synchronize()
    res["obs_quads_first_call_ms"] = float(a.elapsed_time(b))
    res["overhead_ms"] = res["variance_reductions"]["median_ms"] - res["update_llks"]["median_ms"]
    res["overhead_rel"] = res["overhead_ms"] / res["update_llks"]["median_ms"]
    res["shape"] = dict(chains=C, T=spec.T, N=spec.N, P=spec.P, D=spec.D, S=spec.S, covariance=spec.covariance,
                        geodetic_nobs=list(spec.geodetic_nobs or ()), library_GB=spec.lib_bytes / 1e9,
                        kernel=ctx.last_kernel())
    f.release()
    del prob, host, f
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    return res


def moments_leg(C=512, M=64 * 4096):
    X = torch.randn((C, M), dtype=torch.float64, device=dev)
    Y = torch.empty_like(X)
    state = torch.empty((5, M), dtype=torch.float64, device=dev)
    nbytes = C * M * 8
    res = alternate({"ensemble_moments": lambda: ctx.ensemble_moments_update(X, state, 0),
                     "copy_d2d": lambda: Y.copy_(X)}, args.reps, max(args.iters, 20))
    for k in ("ensemble_moments", "copy_d2d"):
        res[k]["GBps_of_C_M_8_bytes"] = nbytes / (res[k]["median_ms"] * 1e-3) / 1e9
    res["moments_rate_over_copy_rate"] = res["copy_d2d"]["median_ms"] / res["ensemble_moments"]["median_ms"]
    res["shape"] = dict(rows=C, columns=M, bytes=nbytes,
                        note="the copy reads and writes C*M*8 bytes each, the moments kernel reads them once; both rates "
                             "are C*M*8 bytes over the call's time")
    return res


out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters}
out["ensemble_moments"] = moments_leg()
out["config4_N120"] = vr_leg(SyntheticSpec((10, 10), (20, 20), (2.0, 2.0), T=35, N=120, D=2, S=60, st_dt=0.5,
                                           slip_varnames=("uparr", "uperp"), covariance="toeplitz", station_shifts=True,
                                           geodetic_nobs=(214, 214), vel_bounds=(3.0, 4.0), time_bounds=(0.0, 2.0)))
if not args.skip_config3:
    out["config3"] = vr_leg(SyntheticSpec((20,), (20,), (1.0,), T=64, N=4096, D=3, S=25, covariance="scalar",
                                          nuc_margin=0.0, time_bounds=(0.0, 0.0)))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
