"""
Times the device producer of the seismic FFI library (beat_amd/seislib.py, csrc/seislib.hip) on the GPU, and the same
build by its numpy restatement (tests/seislib_ref.py: _process_patch_seismic's loop) on that box's host:

  config4   35 targets x 400 patches x 2 durations x 60 starttimes x 120 samples (1.6 GB), elementary traces of 220 samples
  bench     64 x 400 x 3 x 25 x 4096 (62.9 GB), elementary traces of 4200 samples

Both at deltat = 0.5 s with the reference's default filter (stepwise Butterworth, order 4: a highpass with demean, then a
lowpass).  The elementary responses are random numbers already in HBM: the times are those of the producer alone.

Per shape: ``reps`` calls of ``seis_library_fill`` into one preallocated library after a warm-up call, each between HIP
events (median, min, max); the time per kernel from the context's own event timers (``Context.kernel_time``) in a further
call; the window writer's bytes (the library's size: every byte is written once) per second as a fraction of the 8 TB/s
HBM peak; one ``construct_seismic_library`` from the host-side tables to the adopted tensor on the wall clock.  The host
figure times the numpy loop on ``--host-patches`` patches and SCALES it to all patches (marked as scaled); the rows of
those patches are also compared with the device's, bit for bit, at the size that is timed.

    python tools/time_seislib.py [--out profiles/seislib_timing.json] [--reps 3] [--shapes config4,bench]
"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seislib_timing.json"))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--shapes", default="config4,bench")
ap.add_argument("--host-patches", type=int, default=1)
args = ap.parse_args()

import torch  # noqa: E402

import beat_amd  # noqa: E402
import seislib_ref as ref  # noqa: E402
from beat_amd import seislib as sl, seislib_binding as sb  # noqa: E402
from beat_amd.ffi import SeismicGFLibrary, SeismicGFLibraryConfig  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
dev = torch.device("cuda", 0)
HBM_PEAK = 8.0e12
DELTAT = 0.5
FILTERER = sl.Filter(0.01, 0.4, order=4, stepwise=True)
KERNELS = ("stf_table", "stf_convolve", "trace_filter", "lib_windows")
SHAPES = OrderedDict(
    config4=dict(T=35, P=400, L=220, durations=np.array([1.0, 1.5]), starttimes=np.arange(60) * 0.5,
                 taper=sl.ArrivalTaper(-15.0, -10.0, 50.0, 55.0)),
    bench=dict(T=64, P=400, L=4200, durations=np.array([1.0, 1.5, 2.0]), starttimes=np.arange(25) * 0.5,
               taper=sl.ArrivalTaper(-15.0, -10.0, 2038.0, 2043.0)))


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), n=len(v))


def run(name, T, P, L, durations, starttimes, taper):
    D, S, N = durations.size, starttimes.size, taper.nsamples(1.0 / DELTAT)
    print("== %s: %d x %d x %d x %d x %d, L = %d" % (name, T, P, D, S, N, L), flush=True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    X = torch.randn((T, P, L), dtype=torch.float64, device=dev, generator=gen)
    rng = np.random.default_rng(5)
    tmins = 20.0 + rng.integers(-8, 9, (T, P)) * DELTAT
    arrivals = 40.0 + rng.integers(0, 20, T) * DELTAT
    stages = sl.filter_stages(FILTERER, DELTAT)
    i0, w0 = sl.window_tables(tmins, arrivals, starttimes, DELTAT, taper)
    nt, A = sb.stf_table(ctx, durations, DELTAT, like=X)
    lib = torch.empty((T, P, D, S, N), dtype=torch.float64, device=dev)
    i0d, w0d = torch.from_numpy(i0).to(dev), torch.from_numpy(w0).to(dev)
    nbytes = lib.numel() * 8
    case = OrderedDict(case=name, T=T, P=P, D=D, S=S, N=N, L=L, library_bytes=int(nbytes), stages=len(stages),
                       nt=nt.cpu().numpy().tolist())

    def fill():
        sb.seis_library_fill(ctx, X, nt, A, stages, i0d, w0d, N, out=lib)

    fill()                                              # warm-up: code objects, the intermediate buffer's first allocation
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fill()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    case["seis_library_fill"] = stats(times)
    ctx.enable_timing(True)
    ctx.reset_timing()
    fill()
    torch.cuda.synchronize()
    per = OrderedDict()
    for k in KERNELS[1:]:
        ms, n = ctx.kernel_time(k)
        per[k] = dict(total_ms=float(ms), launches=int(n))
    ctx.reset_timing()
    sb.stf_table(ctx, durations, DELTAT, like=X)
    torch.cuda.synchronize()
    ms, n = ctx.kernel_time("stf_table")
    per["stf_table"] = dict(total_ms=float(ms), launches=int(n))
    ctx.enable_timing(False)
    case["kernels"] = per
    wms = per["lib_windows"]["total_ms"]
    case["window_writer_bytes_per_s"] = float(nbytes / (wms * 1e-3))
    case["window_writer_fraction_of_8TBps"] = float(nbytes / (wms * 1e-3) / HBM_PEAK)
    print(json.dumps(case), flush=True)

    # the host route on a few patches, scaled; and the device's rows of those patches against it
    hp = min(args.host_patches, P)
    Xh = X[:, :hp].cpu().numpy()
    nth, Ah = nt.cpu().numpy(), A.cpu().numpy()
    twin = SeismicGFLibrary(SeismicGFLibraryConfig(
        dimensions=(T, hp, D, S, N), starttime_sampling=0.5, duration_sampling=0.5, starttime_min=float(starttimes.min()),
        duration_min=float(durations.min())))
    twin.setup(T, hp, D, S, N, allocate=True)
    t0 = time.perf_counter()
    ref.build_library(twin, Xh, tmins[:, :hp], DELTAT, arrivals, durations, starttimes, (taper.a, taper.b, taper.c, taper.d),
                      stages, nth, Ah)
    host_s = time.perf_counter() - t0
    case["host_numpy_patches_timed"] = hp
    case["host_numpy_s_for_those_patches"] = float(host_s)
    case["host_numpy_s_all_patches_SCALED"] = float(host_s * P / hp)
    case["device_rows_equal_host_rows"] = bool(np.array_equal(lib[:, :hp].cpu().numpy(), twin._gfmatrix))
    del lib, twin
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    gfs = sl.construct_seismic_library(X, tmins, DELTAT, arrivals, durations, starttimes, taper, FILTERER, ctx=ctx)
    torch.cuda.synchronize()
    case["construct_seismic_library_wall_s"] = float(time.perf_counter() - t0)
    del gfs
    torch.cuda.empty_cache()
    print(json.dumps(case), flush=True)
    return case


out = OrderedDict(device=torch.cuda.get_device_name(0), reps=args.reps, deltat=DELTAT, hbm_peak_bytes_per_s=HBM_PEAK,
                  filter="Filter(0.01, 0.4, order=4, stepwise=True): 2 stages of 5 taps", cases=[])
for name in args.shapes.split(","):
    out["cases"].append(run(name, **SHAPES[name]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print("wrote", args.out)
