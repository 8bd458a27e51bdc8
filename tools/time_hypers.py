"""Times a hyper-parameter run (beat_amd/models/hypers.py) three ways in one process, alternating, three runs each,
device work closed by a synchronise:

  (a) steps   the step-by-step path, eager: draw, propose, k_hyper_logp, accept, tune -- one launch each
  (b) graph   the same in the graph chunks BatchedMetropolis.run(use_graph=True) builds
  (c) launch  chain_batch: the whole run in ONE launch of k_hyper_chain

at the reference's default (20 chains x 25 000 steps, 3 hyper-parameters), at 512 and 4096 chains, and at 70
hyper-parameters.  (a) / (b) consist of kernels that existed before plus the trivial k_hyper_logp: what the feature
costs without the new kernel.  No trace is recorded in any mode.

    python tools/time_hypers.py [--steps 25000] [--out profiles/hypers_timing.json] [--only launch]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def case(nh, terms_per_h=4, seed=3):
    rng = np.random.default_rng(seed + nh)
    nterm = nh * terms_per_h
    M = rng.integers(30, 501, nterm)
    llk = M * np.exp(2.0 * rng.uniform(-1.0, 3.0, nterm))
    slog = rng.uniform(-50.0, 50.0, nterm)
    return dict(nh=nh, M=M, slog=slog, kind=np.zeros(nterm, dtype=np.int32), hp_index=np.arange(nterm, dtype=np.int32) % nh,
                group_end=[nterm // 2, nterm], llk=llk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=25000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="steps | graph | launch")
    ap.add_argument("--shapes", default="20x3,512x3,4096x3,20x70")
    args = ap.parse_args()
    import torch

    import beat_amd
    from beat_amd.models import HyperModel
    from beat_amd.sampler.metropolis import BatchedMetropolis
    ctx = beat_amd.get_context(0)
    dev = torch.device("cuda", ctx.device)
    modes = [m for m in ("launch", "steps", "graph") if args.only in (None, m)]
    rows = []
    for shape in args.shapes.split(","):
        C, nh = (int(x) for x in shape.split("x"))
        cs = case(nh)
        lower, upper = np.full(nh, -20.0), np.full(nh, 20.0)
        hm = HyperModel.from_tables(nh, cs["M"], cs["slog"], cs["kind"], cs["hp_index"], cs["group_end"], lower=lower,
                                    upper=upper, ctx=ctx)
        hm.set_llks(torch.from_numpy(np.broadcast_to(cs["llk"], (C, cs["llk"].size)).copy()).to(dev))
        H0 = torch.from_numpy(np.random.default_rng(1).uniform(-2.0, 4.0, (C, nh))).to(dev)
        times = {m: [] for m in modes}
        acc = {}
        failed = {}
        for rep in range(args.repeats + 1):          # (the first round warms up: allocations, code objects)
            for mode in modes:
                if mode in failed:
                    continue
                step = BatchedMetropolis(hm, lower, upper, C, device=dev, tune=True, tune_interval=50, scale=1.0, seed=77)
                step.set_proposal(None, "Normal")
                step.use_chain_batch = mode == "launch"
                H = H0.clone()
                L = step.evaluate(H)
                n_acc = torch.zeros((), dtype=torch.int64, device=dev)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                try:
                    step.run(H, L, 1.0, args.steps, n_acc, use_graph=(mode == "graph"))
                    torch.cuda.synchronize(dev)
                except Exception as exc:       # noqa: BLE001 (reported in the table)
                    failed[mode] = "%s: %s" % (type(exc).__name__, exc)
                    continue
                dt = time.perf_counter() - t0
                if rep > 0:
                    times[mode].append(dt * 1e3)
                acc[mode] = (int(n_acc.item()), H.cpu().numpy())
        ref = acc.get("launch") or acc.get("steps")
        for mode in modes:
            t = times[mode]
            row = dict(chains=C, nh=nh, nterm=int(cs["llk"].size), steps=args.steps, mode=mode)
            if t:
                row.update(ms_per_run=float(np.median(t)), us_per_step=float(np.median(t)) * 1e3 / args.steps,
                           spread_ms=[float(min(t)), float(max(t))], runs_ms=[float(x) for x in t],
                           accepted=acc[mode][0], same_end_points_as_first_mode=bool(np.array_equal(acc[mode][1], ref[1])))
            if mode in failed:
                row["failed"] = failed[mode]
            rows.append(row)
            print(json.dumps(row), flush=True)
        hm.release()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(what="tools/time_hypers.py: ms per run of n steps, median of the repeats after one warm-up round",
                           rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
