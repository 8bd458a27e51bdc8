"""Times of the PT proposal adaptation (csrc/ptadapt.hip) on one MI355X, one process:

    moments   one ``beatamd_group_moments_update`` (k_gm_weights + k_gm_s1 + k_gm_s2) at (G, R, n) = (32, 256, 1204), the
              BASELINE config 5 shape, and (8, 64, 120); achieved FLOP/s (2 R n (n + 1) / 2 per group for S2 in its lower
              triangle, 2 R n for S1) and bytes/s (the accumulators read and written once, the R rows read once)
    factor    one ``beatamd_group_moments_factor`` (finish + batched Cholesky) at the same shapes
    pt_step   the PT step of a small synthetic FFI problem (6 temperatures x 8 replicas) with update_proposal off and on,
              alternated in the same process

    python tools/time_pt_adapt.py [--out profiles/pt_adapt_timing.json] [--reps 5]

Each figure: one warm-up, then ``reps`` rounds of ``calls`` back-to-back calls between host clocks around device
synchronisations; reported per call: the median of the rounds with min and max.  Nothing gates on these numbers.  The default
path against the parent commit is bench.py's pt_leg, run on both builds in one session (not part of this tool)."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pt_adapt_timing.json"))
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

import torch  # noqa: E402

import beat_amd  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
dev = torch.device("cuda", 0)


def timed(fn, calls):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls)
    return dict(median_s=float(np.median(out)), min_s=float(min(out)), max_s=float(max(out)), calls=calls, reps=args.reps)


def moments(G, R, n, calls):
    rng = np.random.default_rng(1)
    Q = torch.from_numpy(10.0 + 0.1 * rng.standard_normal((G * R, n))).to(dev)
    like = torch.from_numpy(-5.0 * rng.uniform(size=G * R)).to(dev)
    state = torch.zeros((G, ctx.group_moments_stride(n)), dtype=torch.float64, device=dev)
    ref = torch.zeros((G, n), dtype=torch.float64, device=dev)
    ctx.group_moments_reset(state, n, Q, ref)
    up = timed(lambda: ctx.group_moments_update(state, Q, like, ref), calls)
    flops = G * (R * n * (n + 1) + 2.0 * R * n)
    nbytes = 8.0 * G * (2 * (n * (n + 1) / 2 + n) + R * n)
    up.update(flops=flops, bytes=nbytes, tflops=flops / up["median_s"] / 1e12, tbytes_per_s=nbytes / up["median_s"] / 1e12)
    # enough samples for a covariance that factors
    for _ in range(max(0, (2 * n) // R + 1)):
        Q.add_(0.1 * torch.from_numpy(rng.standard_normal((G * R, n))).to(dev))
        ctx.group_moments_update(state, Q, like, ref)
    F = torch.zeros((G, n, n), dtype=torch.float64, device=dev)
    fa = timed(lambda: ctx.group_moments_factor(state, n, F), max(1, calls // 10))
    _, _, flags = ctx.group_moments_factor(state, n, F)
    fa["flags"] = flags.cpu().numpy().tolist()
    return dict(G=G, R=R, n=n, update=up, factor=fa)


def pt_step():
    import _ptadapt_gpu_worker as w
    f, lo, up = w.build(ctx)
    out = {"off": [], "on": []}
    for rep in range(args.reps + 1):
        for key, on in (("off", False), ("on", True)):
            _, _, man = w.run_pt(f, lo, up, dev, n_samples=16 * 40, update_proposal=on)
            if rep:
                out[key].append(man.loop_seconds / man.loop_steps)
    return {k: dict(median_s=float(np.median(v)), min_s=float(min(v)), max_s=float(max(v)), reps=args.reps)
            for k, v in out.items()}


res = dict(device=torch.cuda.get_device_name(0), moments=[moments(32, 256, 1204, 20), moments(8, 64, 120, 200)],
           pt_step=pt_step())
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res, indent=1))
