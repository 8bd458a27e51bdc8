"""
Times the mechanism-ensemble arrays on the GPU against the numpy restatement of the loop they replace, on the same box:

  fuzzy_beachball    mts2amps of 4096 and of 10^5 draws, "full", grid 100 (draw_fuzzy_beachball)
  fuzzy_mt_decomp    decomposition_amps of 4096 draws, five parts, grid 400 (fuzzy_mt_decomposition)
  hudson             hudson_project of 10^5 draws (draw_hudson)
  host               the restatement of tests/mechanisms_ref.py (numpy.linalg.eigh per draw, one matrix-vector product per
                     draw and part); for more than 512 draws 512 are timed and the figure is scaled, marked as such

Device times: HIP events around ``iters`` calls after a warm-up call, ``iters`` chosen so that a window lasts about half a
second; medians over ``reps`` windows.  For the count kernel its own time (``Context.kernel_time``) and the fraction of the
FP64 vector rate (256 CUs x 64 lanes x 2.4 GHz lane-instructions per second) that the number of (pixel, draw) terms
implies, with the vector instructions per term counted in the ISA of the inner loop (hipcc -S): 218 per 16 terms in the
wide shape (176 FP64 products and sums, 16 FP64 compares, 26 integer), 60 per 4 in the narrow one.

One process; every step runs under an alarm of its own, and a step that runs out ends the run: nothing more is started on
the device, and what was measured so far is written.

    python tools/time_mechanisms.py [--out profiles/mechanisms_timing.json] [--reps 3] [--step-seconds 120]
"""
import argparse
import json
import os
import signal
import sys
import time
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mechanisms_timing.json"))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--step-seconds", type=int, default=120)
args = ap.parse_args()

import torch  # noqa: E402

import beat_amd  # noqa: E402
import mechanisms_ref as ref  # noqa: E402
from beat_amd import mechanisms as M  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
dev = torch.device("cuda", 0)
FP64_LANE_INSTR_PER_S = 256 * 64 * 2.4e9
VALU_PER_TERM = {"wide": 218.0 / 16.0, "narrow": 60.0 / 4.0}
HOST_DRAWS = 512


class StepTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise StepTimeout()


signal.signal(signal.SIGALRM, _alarm)


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), n=len(v))


def device_time(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    iters = int(min(max(0.5 / max(time.perf_counter() - t0, 1e-6), 1), 200))
    out = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    d = stats(out)
    d["iters"] = iters
    return d


def host_time(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def count_kernel(fn, terms, shape):
    ctx.enable_timing(True)
    ctx.reset_timing()
    fn()
    torch.cuda.synchronize()
    ms, n = ctx.kernel_time("fuzzy_count")
    dms, dn = ctx.kernel_time("mt_decompose")
    ctx.enable_timing(False)
    per = ms / max(n, 1)
    return OrderedDict(kernel_ms=float(per), launches=int(n), decompose_kernel_ms=float(dms / max(dn, 1)), terms=float(terms),
                       shape=shape, valu_per_term=VALU_PER_TERM[shape],
                       fp64_vector_fraction=float(terms * VALU_PER_TERM[shape] / (per * 1e-3) / FP64_LANE_INSTR_PER_S))


def launch_shape(npix, n, P):
    """the launcher's choice (csrc/mechanisms.hip launch_fuzzy_amps)"""
    return "wide" if -(-npix // 1024) * -(-n // 512) * P >= 512 else "narrow"


def host_mts2amps(mts, res, rw, parts):
    """the reference's loop restated: per draw one decomposition, per part one (npix, 6) . (6,) product and a threshold"""
    acc = np.zeros((len(parts), rw.shape[1]))
    for m in mts:
        pa = ref.standard_decomposition(m)[2]
        for k, p in enumerate(parts):
            a = rw.T.dot(ref.unit6(pa[p]))
            acc[k] += a > 0
    return acc / len(mts)


def beachball_case(n, res=100):
    mts = np.random.default_rng(n).normal(size=(n, 6))
    Xd = torch.from_numpy(mts).to(dev)
    rw, pix, _, _ = M.focal_sphere(res, "lambert", "any_P")
    case = OrderedDict(case="fuzzy_beachball", draws=n, grid=res, pixels=int(pix.size))
    case["mts2amps"] = device_time(lambda: M.mts2amps(Xd, "lambert", "full", res))
    case["mts2amps_host_arrays"] = device_time(lambda: M.mts2amps(mts, "lambert", "full", res))
    case["k_fuzzy_count"] = count_kernel(lambda: M.mts2amps(Xd, "lambert", "full", res), float(n) * pix.size,
                                         launch_shape(pix.size, n, 1))
    k = min(n, HOST_DRAWS)
    ms = host_time(lambda: host_mts2amps(mts[:k], res, rw, (4,)))
    case["host_numpy_draws_timed"], case["host_numpy_ms"], case["host_numpy_scaled_ms"] = k, ms, ms * n / k
    return case


def decomposition_case(n, res=400):
    mts = np.random.default_rng(n + 1).normal(size=(n, 6))
    Xd = torch.from_numpy(mts).to(dev)
    rw, pix, _, _ = M.focal_sphere(res, "lambert", "any_P")
    case = OrderedDict(case="fuzzy_mt_decomp", draws=n, grid=res, pixels=int(pix.size), parts=5)
    case["decomposition_amps"] = device_time(lambda: M.decomposition_amps(Xd, res))
    case["k_fuzzy_count"] = count_kernel(lambda: M.decomposition_amps(Xd, res), 5.0 * n * pix.size,
                                         launch_shape(pix.size, n, 5))
    k = min(n, 64)
    ms = host_time(lambda: host_mts2amps(mts[:k], res, rw, (0, 1, 2, 3, 4)))
    case["host_numpy_draws_timed"], case["host_numpy_ms"], case["host_numpy_scaled_ms"] = k, ms, ms * n / k
    return case


def hudson_case(n):
    mts = np.random.default_rng(n + 2).normal(size=(n, 6))
    Xd = torch.from_numpy(mts).to(dev)
    case = OrderedDict(case="hudson", draws=n)
    case["hudson_project"] = device_time(lambda: M.hudson_project(Xd))
    case["hudson_project_host_arrays"] = device_time(lambda: M.hudson_project(mts))
    k = min(n, 4096)
    ms = host_time(lambda: [ref.hudson_of(m) for m in mts[:k]])
    case["host_numpy_draws_timed"], case["host_numpy_ms"], case["host_numpy_scaled_ms"] = k, ms, ms * n / k
    return case


STEPS = [("fuzzy_beachball 4096", lambda: beachball_case(4096)), ("fuzzy_beachball 100000", lambda: beachball_case(100000)),
         ("fuzzy_mt_decomp 4096", lambda: decomposition_case(4096)),
         ("fuzzy_mt_decomp 100000", lambda: decomposition_case(100000)), ("hudson 100000", lambda: hudson_case(100000))]

out = OrderedDict(device=torch.cuda.get_device_name(0), reps=args.reps, fp64_lane_instr_per_s=FP64_LANE_INSTR_PER_S,
                  step_seconds=args.step_seconds, cases=[])
for name, step in STEPS:
    print("== %s" % name, flush=True)
    signal.alarm(args.step_seconds)
    try:
        case = step()
    except StepTimeout:
        out["stopped_at"] = name
        print("   ran out of its %d s: nothing more is started" % args.step_seconds, flush=True)
        break
    finally:
        signal.alarm(0)
    print(json.dumps(case), flush=True)
    out["cases"].append(case)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", args.out)
sys.exit(1 if "stopped_at" in out else 0)
