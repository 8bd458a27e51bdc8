"""Times of the rupture-front arrays (csrc/rupture.hip) on one MI355X, one process, legs alternated:

  1000 draws of one 20 x 20 subfault of 1 km patches (start times from the device's own sweep of random velocities and
  hypocentres) contoured at matplotlib's automatic levels and drawn into 475 x 475 pixels at line width 7 -- what
  ``fault_slip_distribution`` / ``fuzzy_rupture_fronts`` (plotting/ffi.py:338-398, :599-615) do for one subfault.
    minmax            k_rupture_minmax and the copy of (E, 1, 2) doubles to the host
    auto_levels       matplotlib's level rule on the host, E times (Python floats)
    contour_lines     k_contour_count, the scan on the host, k_contour_fill
    polyline_density  k_polyline_check and k_polyline_density over the lines of all draws
    whole             ``start_time_contours`` and ``polyline_density``: all of the above
  the kernels alone from HIP events on the launch stream (``Context.kernel_time``) in a round of their own, the density at
  other tile shapes (``--tiles``, BEATAMD_PD_STRIP x BEATAMD_PD_ROWS), and the host route on ``--host-draws`` of the same
  draws: matplotlib's ``ax.contour`` per draw where matplotlib is importable, and the numpy restatement of the drawing
  (tests/rupture_ref.py, the arithmetic of ``draw_line_on_array``).

    python tools/time_rupture.py [--out profiles/rupture_timing.json] [--reps 3] [-E 1000] [--host-draws 20]

Each leg: a warm-up call, then ``reps`` rounds in which the legs are timed one after the other (wall clock around a
synchronised call); reported: the median of the rounds with min and max.  Nothing gates on these numbers."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rupture_timing.json"))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("-E", type=int, default=1000)
ap.add_argument("--host-draws", type=int, default=20)
ap.add_argument("--tiles", default="32x4096,8x64,64x64,128x128")
args = ap.parse_args()
os.environ.setdefault("BEATAMD_KNOBS_LIVE", "1")       # the tile legs flip BEATAMD_PD_* between calls

import torch  # noqa: E402

import beat_amd  # noqa: E402
from beat_amd import rupture as R, rupture_binding as rb  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
ctx.use_torch_stream()
dev = torch.device("cuda", 0)
ND = NS = 20
PSIZE, LW = 1.0, 7
E = args.E


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


rng = np.random.default_rng(20261021)
slow = torch.from_numpy(1.0 / rng.uniform(2.0, 4.0, (E, ND * NS))).to(dev)
sts = ctx.fast_sweep_batch(slow, PSIZE, rng.integers(0, NS, E).astype(np.int32), rng.integers(0, ND, E).astype(np.int32), NS, ND)
x, y = PSIZE / 2 + PSIZE * np.arange(NS), PSIZE / 2 + PSIZE * np.arange(ND)
extent, shape = R.front_grid(x, y)
subs = rb.subfault_table(ND, NS)
xs, ys = rb.check_coordinates(x, y, subs)
minmax = rb.rupture_minmax(ctx, sts, subs)
lv, nl = R._level_tables(None, E, 1, minmax)
vertices, line_offsets, level_offsets = rb.contour_lines(ctx, sts, subs, xs, ys, lv, nl)
grid = torch.zeros(shape, dtype=torch.float64, device=dev)
cov = torch.zeros(shape, dtype=torch.int32, device=dev)


def density(tile=None):
    def run():
        for k, v in zip(("BEATAMD_PD_STRIP", "BEATAMD_PD_ROWS"), tile or (None, None)):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        rb.polyline_density(ctx, vertices, line_offsets, extent, shape, LW, grid, cov)
        os.environ.pop("BEATAMD_PD_STRIP", None)
        os.environ.pop("BEATAMD_PD_ROWS", None)
    return run


def whole():
    c = R.start_time_contours(sts, ND, NS, x, y, ctx=ctx)
    rb.polyline_density(ctx, c["vertices"], c["line_offsets"], extent, shape, LW)


legs = {"minmax": lambda: rb.rupture_minmax(ctx, sts, subs),
        "auto_levels": lambda: R._level_tables(None, E, 1, minmax),
        "contour_lines": lambda: rb.contour_lines(ctx, sts, subs, xs, ys, lv, nl),
        "polyline_density": density(), "whole": whole}
for t in [v for v in args.tiles.split(",") if v]:
    legs["polyline_density_tile_%s" % t] = density(tuple(int(v) for v in t.split("x")))
res = alternate(legs, args.reps)

# the kernels alone, from events on the launch stream
ctx.enable_timing(True)
ctx.reset_timing()
for _ in range(args.reps):
    rb.contour_lines(ctx, sts, subs, xs, ys, lv, nl)
    density()()
torch.cuda.synchronize()
kernels = {}
for name in ("contour_count", "contour_fill", "polyline_density"):
    ms, n = ctx.kernel_time(name)
    kernels[name] = dict(mean_ms=ms / max(n, 1), launches=n)
ctx.enable_timing(False)

nlines, nverts = int(line_offsets.shape[0]) - 1, int(vertices.shape[0])
out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "legs": res, "kernels_event_ms": kernels,
       "shape": dict(E=E, subfault=[ND, NS], grid=list(shape), linewidth=LW, lines=nlines, vertices=nverts,
                     levels_per_draw=float(nl.mean()), segments=nverts - nlines,
                     coverage_nonzero_fraction=float((cov.cpu().numpy() != 0).mean()),
                     note="wall clock around one synchronised call; polyline_density (k_polyline_check + k_polyline_density) "
                          "reports errors and so synchronises itself; kernels_event_ms brackets the launches of an entry")}

# the host route on a few of the same draws
H = min(args.host_draws, E)
if H > 0:
    import rupture_ref as rref
    sts_h = sts[:H].cpu().numpy()
    host = {}
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        fig, ax = plt.subplots()
        xg, yg = np.meshgrid(x, y)
        t0 = time.perf_counter()
        fronts = [ax.contour(xg, yg, sts_h[e].reshape(ND, NS)).allsegs for e in range(H)]
        host["matplotlib_contour_ms_per_draw"] = (time.perf_counter() - t0) * 1e3 / H
        plt.close(fig)
    except ImportError:
        fronts = None
    t0 = time.perf_counter()
    v, lo, lvl = rref.contours(sts_h, [ND], [NS], [x], [y], [[lv[e, 0, :nl[e, 0]]] for e in range(H)])
    host["restated_contours_ms_per_draw"] = (time.perf_counter() - t0) * 1e3 / H
    t0 = time.perf_counter()
    g_h, c_h = rref.polyline_density(v, lo, extent, shape, LW)
    host["restated_drawing_ms_per_draw"] = (time.perf_counter() - t0) * 1e3 / H
    g_d, c_d = rb.polyline_density(ctx, vertices, line_offsets, extent, shape, LW,
                                   lines=np.arange(int(level_offsets[H - 1, 0, -1]), dtype=np.int64))
    host["device_equals_restatement_on_these_draws"] = bool(np.array_equal(g_d.cpu().numpy(), g_h)
                                                            and np.array_equal(c_d.cpu().numpy(), c_h))
    host["draws"] = H
    per_draw = host.get("matplotlib_contour_ms_per_draw", host["restated_contours_ms_per_draw"]) + host["restated_drawing_ms_per_draw"]
    host["host_route_ms_per_draw"] = per_draw
    host["host_route_s_for_E_draws"] = per_draw * E / 1e3
    out["host_route"] = host

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
