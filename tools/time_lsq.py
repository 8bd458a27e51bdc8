"""Times of the least-squares start (LogpForwFunc.lsq_solution, csrc/lsq.hip) on one MI355X, one process, 512 chains, at
two shapes (patches x targets x samples):

    joint     400 x 35 x 120 seismic, two geodetic datasets of 214 and 205 points, laplacian
    config3   400 x 64 x 4096 seismic (the 62.9 GB library of BASELINE config 3, generated on the device), laplacian

    python tools/time_lsq.py [--out profiles/lsq_timing.json] [--reps 3] [--chains 512] [--skip-config3]

Device leg: one warm-up call, then ``reps`` calls between host clocks around device synchronisations, with the library's
event timers on, so each call is split into index tables, Gram matrices (k_lsq_gram), right-hand side (k_lsq_rhs),
chain-independent blocks (k_lsq_finish) and the active set (k_nnls); reported: medians with min and max.  The Gram kernel's
useful rate counts the lower triangle only: chains x P (P + 1) / 2 x 2 x T x N flop.

Host leg (the joint shape only; the config3 library does not fit host memory): the reference's route on this machine's CPU
for a few chains -- one gather of the whole library per patch (what stack_all(patchidxs=[p]) reads in numpy mode), the
stacked design matrix, scipy.optimize.nnls -- and its extrapolation to all chains (chains are independent: x chains / n).
For config3 the host figure is the joint one scaled by the ratio of the seismic rows (T N), stated as such.  Nothing gates on
these numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsq_timing.json"))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--chains", type=int, default=512)
ap.add_argument("--host-chains", type=int, default=2)
ap.add_argument("--skip-config3", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

import beat_amd  # noqa: E402
from beat_amd.synthetic import SyntheticSpec, build_problem  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
KERNELS = ("tables", "lsq_gram", "lsq_rhs", "lsq_finish", "nnls")


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), n=len(v))


def clocked(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def population(prob, host, n):
    lo, up = host["layout"].bounds(host["lower"], host["upper"])
    rng = np.random.RandomState(1)
    return lo + (up - lo) * rng.random_sample((n, lo.size))


def host_route(prob, host, Q, st0):
    """the reference's route for the chains of Q on the CPU -> milliseconds per chain"""
    from scipy.optimize import nnls
    spec, lay = host["spec"], host["layout"]
    G = host["Gs"][0]
    T, P, D, S, N = G.shape
    tt = np.arange(T)
    t0 = time.perf_counter()
    for c in range(Q.shape[0]):
        pt = lay.rmap(Q[c])
        di = np.round((pt["durations"] - spec.du_min) / spec.du_dt).astype("int16")
        si = np.round((st0[c][None, :] - spec.st_min) / spec.st_dt).astype("int16")
        cols = [G[tt, p, di[p], si[:, p], :].reshape(T * N) for p in range(P)]
        rows = [np.stack(cols, axis=1)]
        rhs = [host["data"].ravel()]
        if spec.geodetic_nobs:
            rows.append(host["gGs"][0].T)
            rhs.append(host["gdata"])
        rows.append(host["L"] * float(pt["h_laplacian"][0]) ** 2.0)
        rhs.append(np.zeros(P))
        nnls(np.vstack(rows), np.hstack(rhs))
    return (time.perf_counter() - t0) * 1e3 / Q.shape[0]


def leg(spec, device_library, with_host):
    prob, host = build_problem(spec, device_library=device_library, ctx=ctx)
    f = prob.compile(ctx)
    Q = population(prob, host, args.chains)
    Qd = torch.from_numpy(Q).cuda()
    f.lsq_solution(Qd)                                   # warm-up (and the chain-independent blocks)
    total, kern = [], {k: [] for k in KERNELS}
    for _ in range(args.reps):
        ctx.enable_timing(True)
        ctx.reset_timing()
        ms, (out, it, st) = clocked(lambda: f.lsq_solution(Qd, return_info=True))
        total.append(ms)
        for k in KERNELS:
            kern[k].append(ctx.kernel_time(k)[0])
        ctx.enable_timing(False)
    P, T, N = spec.P, spec.T, spec.N
    flop = args.chains * P * (P + 1) / 2 * 2.0 * T * N
    gram = stats(kern["lsq_gram"])
    res = dict(shape=dict(P=P, T=T, N=N, chains=args.chains, geodetic=list(spec.geodetic_nobs or ())),
               device_total=stats(total), device_by_kernel={k: stats(v) for k, v in kern.items()},
               gram_useful_tflops=flop / (gram["median_ms"] * 1e-3) / 1e12,
               iterations=dict(mean=float(it.float().mean()), max=int(it.max())), support_mean=float((out[:, :P] > 0).sum(1).float().mean()))
    if with_host:
        n = args.host_chains
        st0 = f.start_times(Q[:n])
        per_chain = host_route(prob, host, Q[:n], st0)
        res["host"] = dict(chains_timed=n, ms_per_chain=per_chain, extrapolated_ms=per_chain * args.chains,
                           note="chains are independent: extrapolated = ms_per_chain x chains (one CPU process)")
        res["host_over_device"] = res["host"]["extrapolated_ms"] / res["device_total"]["median_ms"]
    f.release()
    return res


out = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
out["joint"] = leg(SyntheticSpec((20,), (20,), (1.0,), T=35, N=120, D=3, S=25, slip_varnames=("uparr", "uperp"),
                                 geodetic_nobs=(214, 205), laplacian=True, time_bounds=(0.0, 0.5)), False, True)
if not args.skip_config3:
    out["config3"] = leg(SyntheticSpec((20,), (20,), (1.0,), T=64, N=4096, D=3, S=25, slip_varnames=("uparr",), laplacian=True,
                                       time_bounds=(0.0, 0.5)), True, False)
    rows_j, rows_c = 35 * 120, 64 * 4096
    out["config3"]["host"] = dict(extrapolated_ms=out["joint"]["host"]["extrapolated_ms"] * rows_c / rows_j,
                                  note="not run: the joint shape's host time scaled by the ratio of seismic rows (T N)")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out))
