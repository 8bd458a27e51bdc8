"""Times of the density grids (fuzzy waveforms) on one MI355X, one process, legs alternated:

  ``trace_density_update`` of an ensemble Y [E, T, N] = 200 draws x 64 targets at N = 4096 and at N = 120 samples into
  500 x 500 grids at line width 7 (the reference's defaults, plotting/seismic.py:503), next to what else can be done with
  the same array:
    copy_d2d          a device-to-device copy of its E * T * N * 8 bytes
    ensemble_moments  k_ensemble_moments over it
    copy_d2h          the copy to the host that the grid makes unnecessary (pageable, as ``Tensor.cpu()``; and pinned)
  and the same call at other strip widths (grid columns per workgroup, BEATAMD_TD_STRIP; ``--strips``): the pixels drawn
  stay the same, the segments set up per workgroup and the workgroups per compute unit grow with the number of strips.

    python tools/time_density.py [--out profiles/density_timing.json] [--reps 3] [--only 4096|120] [--strips 8,32]
                                 [--once]

Each leg: a warm-up call, then ``reps`` rounds in which the legs are timed one after the other (wall clock around a
synchronised call); reported: the median of the rounds with min and max.  ``--once``: one density call per N and nothing
else (for a kernel trace).  Nothing gates on these numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_timing.json"))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--only", type=int, default=0)
ap.add_argument("--once", action="store_true")
ap.add_argument("--strips", default="8,32")
ap.add_argument("-E", type=int, default=200)
ap.add_argument("-T", type=int, default=64)
args = ap.parse_args()
os.environ.setdefault("BEATAMD_KNOBS_LIVE", "1")       # the strip legs flip BEATAMD_TD_STRIP between calls

import torch  # noqa: E402

import beat_amd  # noqa: E402
from beat_amd.summary import density_extent  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
ctx.use_torch_stream()
dev = torch.device("cuda", 0)
SIZE, LW = (500, 500), 7


def ensemble(E, T, N, seed=0):
    """waveform-like traces on the device: three sinusoids and noise per trace"""
    g = torch.Generator(device=dev).manual_seed(seed)
    j = torch.arange(N, dtype=torch.float64, device=dev)

    def u(lo, hi):
        return lo + (hi - lo) * torch.rand((E, T, 3, 1), dtype=torch.float64, device=dev, generator=g)

    Y = (u(0.2, 1.0) * torch.sin(2 * np.pi * u(0.5, 6.0) / N * j + u(0, 2 * np.pi))).sum(2)     # 0.5 ... 6 cycles per trace
    return (Y + 0.05 * torch.randn((E, T, N), dtype=torch.float64, device=dev, generator=g)).contiguous()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(legs, reps):
    for fn in legs.values():
        fn()
    ts = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ts[k].append(wall(fn))
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), n=len(v))
            for k, v in ts.items()}


def leg(N):
    E, T = args.E, args.T
    Y = ensemble(E, T, N)
    state, seen = ctx.ensemble_moments_update(Y.view(E, T * N))
    _, _, mn, mx = ctx.ensemble_moments_finish(state, seen)
    tmin = np.zeros(T)
    extent = density_extent(mn.view(T, N), mx.view(T, N), tmin, 1.0)
    tmin_d, ext_d = torch.from_numpy(tmin).to(dev), torch.from_numpy(extent).to(dev)
    grid = torch.zeros((T,) + SIZE, dtype=torch.float64, device=dev)

    def density(strip=None):
        def run():
            if strip is None:
                os.environ.pop("BEATAMD_TD_STRIP", None)
            else:
                os.environ["BEATAMD_TD_STRIP"] = str(strip)
            ctx.trace_density_update(Y, tmin_d, 1.0, ext_d, SIZE, LW, grid)
            os.environ.pop("BEATAMD_TD_STRIP", None)
        return run

    if args.once:
        ms = wall(density())
        return dict(trace_density_once_ms=ms)
    Z = torch.empty_like(Y)
    pinned = torch.empty(Y.shape, dtype=torch.float64, pin_memory=True)
    legs = {"trace_density": density(), "copy_d2d": lambda: Z.copy_(Y),
            "ensemble_moments": lambda: ctx.ensemble_moments_update(Y.view(E, T * N), state, 0),
            "copy_d2h_pageable": lambda: Y.cpu(), "copy_d2h_pinned": lambda: pinned.copy_(Y)}
    for w in [int(v) for v in args.strips.split(",") if v]:
        legs["trace_density_strip%d" % w] = density(w)
    res = alternate(legs, args.reps)
    nbytes = E * T * N * 8
    for k in res:
        res[k]["GBps_of_E_T_N_8_bytes"] = nbytes / (res[k]["median_ms"] * 1e-3) / 1e9
    res["trace_density"]["us_per_trace"] = res["trace_density"]["median_ms"] * 1e3 / (E * T)
    g = grid.cpu().numpy()
    res["shape"] = dict(E=E, T=T, N=N, grid=list(SIZE), linewidth=LW, bytes=nbytes,
                        grid_nonzero_fraction=float((g != 0).mean()),
                        note="wall clock around one synchronised call; the density call reports errors and so "
                             "synchronises itself")
    return res


out = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
       "reference_cpu_s_per_trace": dict(N=4096, grid=[500, 500], linewidth=7, seconds=0.23,
                                         note="draw_line_on_array of the reference on one CPU core, a single run")}
for N in (4096, 120):
    if args.only in (0, N):
        out["N%d" % N] = leg(N)
if not args.once:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
print(json.dumps(out))
