#!/usr/bin/env python
"""Times ``beat_amd.diagnostics.summary`` on the device against the numpy restatement (tests/convergence_ref.py, FFT
autocovariance) on the same machine and writes profiles/convergence_timing.json:

  smc   the 4096 x 100 x 1204 posterior of a thinned SMC stage as ONE chain of 409600 draws (what ``beat summarize`` hands over)
  pt    a 32 x 20000 x 50 trace of slowly mixing chains (AR(1), phi = 0.98)

The host restatement is timed on a few variables and scaled to all of them (it works variable by variable).  The share of
``k_acov_lags`` comes from the context's kernel timers (HIP events around the launches), measured in a run of its own.

    python tools/convergence_timing.py [--reps 3] [--host-vars 4] [--out profiles/convergence_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ts):
    ts = sorted(ts)
    return dict(median_ms=1e3 * ts[len(ts) // 2], min_ms=1e3 * ts[0], max_ms=1e3 * ts[-1], n=len(ts))


def device_ar1(C, D, V, phi, seed):
    """(C, D, V) on the device: stationary unit-variance AR(1) chains (phi = 0: white noise)"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((C, D, V), dtype=torch.float64, device="cuda", generator=g)
    if phi:
        s = float(np.sqrt(1.0 - phi * phi))
        for d in range(1, D):
            x[:, d] = phi * x[:, d - 1] + s * x[:, d]
    return x


def run_case(name, C, D, V, phi, reps, host_vars):
    import torch

    import convergence_ref as ref
    from beat_amd import diagnostics as dg
    from beat_amd.engine import get_context
    X = device_ar1(C, D, V, phi, 11)
    ctx = get_context()
    out = dict(case=name, chains=C, draws=D, variables=V, phi=phi)
    t = dg.summary(X)       # warm-up: allocations, code objects
    torch.cuda.synchronize()
    out["rounds"] = t["rounds"]
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        t = dg.summary(X)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    out["device_summary"] = stats(ts)
    ctx.enable_timing(True)
    ctx.reset_timing()
    dg.summary(X)
    torch.cuda.synchronize()
    total, _ = ctx.kernel_time("convergence_summary")
    lags, launches = ctx.kernel_time("acov_lags")
    sort, _ = ctx.kernel_time("col_sort")
    ctx.enable_timing(False)
    out["kernels"] = dict(convergence_summary_ms=total, k_acov_lags_ms=lags, k_acov_lags_launches=launches,
                          k_acov_lags_share=lags / total if total else None, col_sort_ms=sort,
                          col_sort_share=sort / total if total else None)
    nh = min(host_vars, V)
    Xh = X[:, :, :nh].cpu().numpy()
    t0 = time.perf_counter()
    want = ref.summary(Xh, route="fft")
    host = time.perf_counter() - t0
    out["host_restatement_fft"] = dict(variables=nh, ms=1e3 * host, scaled_to_all_ms=1e3 * host * V / nh)
    out["speedup_vs_host_scaled"] = (host * V / nh) / (out["device_summary"]["median_ms"] * 1e-3)
    got = np.array([t[k].cpu().numpy()[:nh] for k in ("mean", "sd", "ess_bulk", "ess_tail", "r_hat", "ess_mean", "ess_sd")]).T
    out["rel_max_vs_host"] = float(np.nanmax(np.abs(got / want[:, [0, 1, 6, 7, 8, 9, 10]] - 1.0)))
    del X
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-vars", type=int, default=4)
    ap.add_argument("--small", action="store_true", help="a tenth of the draws (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convergence_timing.json"))
    a = ap.parse_args()
    import torch
    f = 10 if a.small else 1
    cases = [run_case("smc", 1, 4096 * 100 // f, 1204, 0.0, a.reps, a.host_vars),
             run_case("pt", 32, 20000 // f, 50, 0.98, a.reps, a.host_vars)]
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, small=bool(a.small), cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
