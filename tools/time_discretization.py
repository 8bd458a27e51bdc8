"""Times the geodetic library fill, one model resolution and one whole optimize_discretization on the device, and the
host numpy restatement (tests/discretization_ref.py, Green's functions from oracle/okada_oracle.py) on the same box, at
a Laquila-sized problem (two scenes, 428 points) and at 4096 points.  Writes profiles/discretization_timing.json.

    python tools/time_discretization.py [--out PATH] [--skip-host-loop-above NOBS]

Device times are the median of five calls after a warm-up, synchronised; host times are single runs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import discretization_ref as dref  # noqa: E402


def problem(nobs):
    """one 24 x 12 km fault dipping 50 degrees under two scenes of nobs points in all"""
    rng = np.random.RandomState(428)
    subfaults = np.array([[1.0, -2.0, 0.5, 140.0, 50.0, -90.0, 24.0, 12.0, 1.0, 0.0]])
    n1 = nobs // 2
    sizes = [n1, nobs - n1]
    east, north = rng.uniform(-30.0, 30.0, nobs), rng.uniform(-30.0, 30.0, nobs)
    los = np.vstack([np.tile([-0.08, 0.38, 0.92], (sizes[0], 1)), np.tile([-0.10, -0.62, 0.78], (sizes[1], 1))])
    odw = rng.uniform(0.5, 2.0, nobs)
    cfg = dict(epsilon=4.0e-3, epsilon_search_runs=1, resolution_thresh=0.999, depth_penalty=3.5, alpha=0.3,
               patch_widths_min=[1.0], patch_widths_max=[3.0], patch_lengths_min=[1.0], patch_lengths_max=[3.0])
    return dict(subfaults=subfaults, east=east, north=north, los=los, odw=odw, sizes=sizes, nu=0.25, cfg=cfg,
                varnames=["uparr", "uperp"])


def median_ms(fn, sync, n=5):
    fn()
    sync()
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def once_ms(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "discretization_timing.json"))
    ap.add_argument("--skip-host-loop-above", type=int, default=100000)
    args = ap.parse_args()
    import torch

    import beat_amd
    from beat_amd import discretization as dz
    from beat_amd.ffi import geo_construct_gf_linear_patches
    from beat_amd.heart import GeodeticDataset, HalfspaceEngine
    ctx = beat_amd.get_context(0)
    sync = torch.cuda.synchronize
    result = {"device": torch.cuda.get_device_name(0), "cases": []}
    for nobs in (428, 4096):
        fp = problem(nobs)
        engine = HalfspaceEngine(nu=fp["nu"], ctx=ctx)
        datasets, o = [], 0
        for n in fp["sizes"]:
            s = slice(o, o + n)
            datasets.append(GeodeticDataset(fp["east"][s] * 1e3, fp["north"][s] * 1e3, fp["los"][s], odw=fp["odw"][s]))
            o += n
        base = dref.patches(fp["subfaults"][0], 24, 12)           # 288 patches of 1 km
        rows = np.vstack([dz.component_parameters(base, c) for c in fp["varnames"]])
        case = {"nobs": nobs, "library_rows": int(len(rows))}
        case["library_fill_ms"] = median_ms(
            lambda: geo_construct_gf_linear_patches(engine, datasets=datasets, patches=rows, device=True), sync)
        case["library_fill_host_ms"], G = once_ms(
            lambda: dref.library(rows, fp["east"], fp["north"], fp["los"], fp["odw"], fp["nu"]))
        P = len(base)
        cen = dref.centers(base)
        L = dref.smoothing_correlated(cen, "gaussian")
        d_g, d_l = torch.from_numpy(np.ascontiguousarray(G[:P])).to("cuda:0"), torch.from_numpy(L).to("cuda:0")
        # (a uniform 1 km cut is far finer than the data resolve: damped more than the loop's epsilon, so that the
        # normal matrix stays numerically positive definite)
        case["resolution_npatches"], case["resolution_epsilon"] = P, 0.05
        case["resolution_ms"] = median_ms(lambda: ctx.model_resolution(d_g, d_l, 0.05), sync)
        case["resolution_host_ms"], _ = once_ms(lambda: dref.resolution(G[:P].T, L, 0.05))
        cfg = dz.ResolutionDiscretizationConfig(**fp["cfg"])

        def loop():
            hist = []
            f, _ = dz.optimize_discretization(cfg, dz.DiscretizedFault(fp["subfaults"]), datasets, fp["varnames"],
                                              engine=engine, history=hist)
            return f.npatches, len(hist)
        loop()
        sync()
        case["optimize_discretization_ms"], (npatch, ngen) = once_ms(loop)
        case["final_npatches"], case["generations"] = int(npatch), int(ngen)
        if nobs <= args.skip_host_loop_above:
            ms, r = once_ms(lambda: dref.optimize(fp["cfg"], fp["subfaults"], fp["east"], fp["north"], fp["los"],
                                                  fp["odw"], fp["nu"], fp["varnames"]))
            case["optimize_discretization_host_ms"] = ms
            case["host_final_npatches"] = int(len(r["params"]))
        result["cases"].append(case)
        print(json.dumps(case))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
