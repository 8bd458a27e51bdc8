"""
Times the polarity composite on the GPU and the numpy restatement of it on the same box:

  logp_batch    one ``f.batch(Q)`` (device tensors in and out) of 512 and 4096 chains at 60 and 500 stations, HIP events
                around ``iters`` calls; beside it the kernel's own time (``Context.kernel_time("polarity")``)
  fused_step    the same problems through the fused Metropolis step of an SMC stage, per step
  numpy         tests/polarity_ref.py ``forward`` on the host arrays, wall clock

The problem is the example project's shape: an ``mtqt`` source with kappa, sigma, h free, w = v = 0, one any_P map with its
sigma fixed at 0.05.  Medians over ``reps`` repetitions, each side's minimum and maximum kept.

    python tools/time_polarity.py [--out profiles/polarity_timing.json] [--reps 5] [--iters 200]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polarity_timing.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--iters", type=int, default=200)
args = ap.parse_args()

import torch  # noqa: E402

import beat_amd  # noqa: E402
import polarity_ref as pref  # noqa: E402
from beat_amd.models import ParameterLayout, PolarityMap, PolarityProblem  # noqa: E402
from beat_amd.sampler import SMC  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
dev = torch.device("cuda", 0)


def problem(n_t):
    rng = np.random.default_rng(n_t)
    lay = ParameterLayout(OrderedDict([("kappa", 1), ("sigma", 1), ("h", 1)]))
    pmap = PolarityMap("any_P", rng.uniform(0.0, np.pi, n_t), rng.uniform(0.0, 2.0 * np.pi, n_t), rng.choice([-1, 1], n_t))
    lower = dict(kappa=0.0, sigma=-np.pi / 2.0, h=0.0)
    upper = dict(kappa=2.0 * np.pi, sigma=np.pi / 2.0, h=1.0)
    prob = PolarityProblem(lay, "mtqt", [pmap], fixed={"w": 0.0, "v": 0.0, "h_any_P_pol_0": 0.05}, lower=lower, upper=upper)
    return prob, lay, lower, upper


def stats(v):
    return dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)), n=len(v))


def time_events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3


out = OrderedDict(device=torch.cuda.get_device_name(0), iters=args.iters, reps=args.reps, cases=[])
for n_t in (60, 500):
    prob, lay, lower, upper = problem(n_t)
    f = prob.compile(ctx)
    lo, up = lay.bounds(lower, upper)
    off, fix = prob.source_tables()
    hoff, hfix = prob.hyper_tables()
    for C in (512, 4096):
        rng = np.random.default_rng(C)
        Q = lo + (up - lo) * rng.random((C, lay.size))
        Qd = torch.from_numpy(Q).to(dev)
        LL = torch.empty((C, f.nllk), dtype=torch.float64, device=dev)
        ctx.use_torch_stream()
        for _ in range(20):
            f.batch(Qd, out=LL)
        torch.cuda.synchronize()
        batch = [time_events(lambda: f.batch(Qd, out=LL), args.iters) for _ in range(args.reps)]
        ctx.enable_timing(True)
        ctx.reset_timing()
        for _ in range(args.iters):
            f.batch(Qd, out=LL)
        torch.cuda.synchronize()
        ms, n = ctx.kernel_time("polarity")
        ctx.enable_timing(False)
        # the fused step of an SMC stage
        step = SMC(f, lo, up, n_chains=C, tune_interval=10, device=dev, random_seed=2)
        Qs = step.initialize_population()
        Ls = step.stepper.evaluate(Qs)
        step.select_end_points(Qs, Ls)
        step.transition()
        step.stage += 1
        step.sample_stage(max(args.iters // 4, 5))
        torch.cuda.synchronize()
        fused = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step.sample_stage(args.iters)
            b.record()
            b.synchronize()
            fused.append(a.elapsed_time(b) / args.iters * 1e3)
        # numpy on the same box
        host = []
        for _ in range(max(args.reps, 3)):
            t0 = time.perf_counter()
            ref = pref.forward("mtqt", Q, off, fix, prob.radiation_weights(), prob.observations(), [n_t], prob.gamma, hoff, hfix)
            host.append((time.perf_counter() - t0) * 1e6)
        got = LL.cpu().numpy()
        assert np.allclose(got, ref, rtol=1e-9, atol=0.0)
        out["cases"].append(OrderedDict(chains=C, stations=n_t, logp_batch=stats(batch),
                                        kernel_us=float(ms / max(n, 1) * 1e3), kernel_launches=int(n),
                                        fused_step=stats(fused), numpy_forward=stats(host),
                                        acceptance=float(step.stage_acceptance[-1]) if step.stage_acceptance else None))
    f.release()
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out))
