"""What the spectrum domain of a seismic wavemap costs on one MI355X, next to the time-domain model of the same problem:

  legs      config4   the short-trace shape of BASELINE config 4: 2 subfaults of 10 x 20 = 400 patches, 35 targets, N = 120
                      (ntrans 128), uparr and uperp, station shifts, multilinear
            config3   one 20 x 20 subfault, 64 targets, N = 4096 (ntrans 4096), uparr, nearest neighbour
            512 chains each, scalar weights in both domains (the dense time-domain operators of config 4 are N x N, the
            spectrum's M x M: another comparison), one seismic wavemap and nothing else
  timed     time      f.batch(Q) of the time-domain model (the path of bench.py, unchanged)
            spectrum  f.batch(Q) of the spectrum-domain model over the SAME libraries: stack to scratch, k_amp_spectrum with
                      the residual option, scalar misfit, epilogue
            kernel    k_amp_spectrum alone, from the context's event timers (beatamd_ctx_kernel_time "amp_spectrum") in a run
                      of its own; "hbm_fraction" = the bytes it has to move (C T N 8 read + C T M 8 written) over its time,
                      as a fraction of the 8 TB/s peak
  also      bound_ratio: largest |device - numpy| / bound per ntrans over the cases of tests/test_gpu_spectrum.py test 1
            (tests/spectrum_ref.py kernel_bound_ratio)

    python tools/spectrum_timing.py [--out profiles/spectrum_timing.json] [--reps 7] [--skip-config3]

One process, the legs alternating, wall clock around a synchronised call, the median of ``reps`` rounds after a warm-up, with
min and max.  Nothing gates on the timings."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_timing.json"))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--chains", type=int, default=512)
ap.add_argument("--skip-config3", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

import beat_amd  # noqa: E402
import spectrum_ref as sr  # noqa: E402
from beat_amd.models import FFIProblem, SeismicWavemap  # noqa: E402
from beat_amd.synthetic import SyntheticSpec, build_problem, draw_population  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
HBM_PEAK = 8.0e12
DELTAT = 0.5


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), n=len(v))


def leg(name, spec, band):
    prob, host = build_problem(spec, device_library=True, ctx=ctx)
    wm = prob.wavemaps[0]
    T, N = wm.data.shape
    wm_s = SeismicWavemap(wm.gfs, wm.data, np.asarray(wm.weights, dtype=np.float64), wm.slog_pdet, wm.hypers, wm.time_shifts,
                          wm.interpolation, wm.name, domain="spectrum", deltat=DELTAT, taper_frequencies=band)
    prob_s = FFIProblem(prob.layout, prob.n_patch_dip, prob.n_patch_strike, prob.patch_sizes, prob.slip_varnames, [wm_s],
                        None, None, prob.lower, prob.upper)
    f_t, f_s = prob.compile(ctx), prob_s.compile(ctx)
    C = args.chains
    Q = torch.from_numpy(draw_population(spec, host["layout"], host["lower"], host["upper"], C)).cuda()
    out_t = torch.empty((C, f_t.nllk), dtype=torch.float64, device="cuda")
    out_s = torch.empty((C, f_s.nllk), dtype=torch.float64, device="cuda")
    fns = dict(time=lambda: f_t.batch(Q, out_t), spectrum=lambda: f_s.batch(Q, out_s))
    for fn in fns.values():            # warm-up: code objects, scratch, the group-size measurement of the stacker
        for _ in range(3):
            fn()
    ts = dict((k, []) for k in fns)
    for _ in range(args.reps):
        for k, fn in fns.items():
            ts[k].append(wall(fn))
    # the kernel alone: event timers on, a run of its own
    ctx.enable_timing(True)
    ctx.reset_timing()
    for _ in range(args.reps):
        fns["spectrum"]()
    ctx.synchronize()
    ms, n = ctx.kernel_time("amp_spectrum")
    ctx.enable_timing(False)
    M = wm_s.nsamples_spectrum
    nbytes = C * T * (N + M) * 8
    k_ms = ms / max(n, 1)
    res = dict(shape=dict(chains=C, targets=T, patches=spec.P, N=N, ntrans=wm_s.ntrans, band_hz=list(band),
                          valid_spectrum_indices=list(wm_s.valid_spectrum_indices), M=M, interpolation=wm.interpolation,
                          slip_variables=len(prob.slip_varnames)),
               time=stats(ts["time"]), spectrum=stats(ts["spectrum"]),
               kernel=dict(ms_per_launch=k_ms, launches=int(n), bytes=nbytes,
                           hbm_fraction=(nbytes / (k_ms * 1e-3)) / HBM_PEAK if k_ms > 0 else None,
                           lds_bytes_per_workgroup=8 * wm_s.ntrans * (4 if wm_s.ntrans <= 512 else 1)))
    res["spectrum_over_time"] = res["spectrum"]["median_ms"] / res["time"]["median_ms"]
    print(name, json.dumps(res), flush=True)
    f_t.release()
    f_s.release()
    for gf in wm.gfs.values():
        if getattr(gf, "lib_id", None) is not None:
            ctx.seis_gflib_destroy(gf.lib_id)
            gf.lib_id = None
        gf._device_tensor = None
    del prob, prob_s, f_t, f_s, Q
    torch.cuda.empty_cache()
    return res


out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "hbm_peak_bytes_per_s": HBM_PEAK,
       "what": "milliseconds per logp_batch of 512 chains, wall clock around a synchronised call (median of the rounds, min, "
               "max); kernel: HIP events around k_amp_spectrum in a separate run",
       "bound_ratio": {}, "legs": {}}
for N in sr.KERNEL_SIZES:
    ntrans, worst, where = sr.kernel_bound_ratio(ctx, N)
    key = str(ntrans)
    if worst >= out["bound_ratio"].get(key, {"ratio": -1.0})["ratio"]:
        out["bound_ratio"][key] = dict(ratio=worst, N=N, rows=where[0], band=where[1])
print("bound_ratio", json.dumps(out["bound_ratio"]), flush=True)

out["legs"]["config4_N120"] = leg("config4_N120", SyntheticSpec(
    (10, 10), (20, 20), (2.0, 2.0), T=35, N=120, D=2, S=60, st_dt=0.5, slip_varnames=("uparr", "uperp"), covariance="scalar",
    station_shifts=True, vel_bounds=(3.0, 4.0), time_bounds=(0.0, 2.0), interpolation="multilinear"), (0.02, 0.5))
if not args.skip_config3:
    out["legs"]["config3_N4096"] = leg("config3_N4096", SyntheticSpec(
        (20,), (20,), (1.0,), T=64, N=4096, D=3, S=25, covariance="scalar", nuc_margin=0.0, time_bounds=(0.0, 0.0)), (0.01, 0.5))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
