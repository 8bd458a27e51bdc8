"""A geodetic composite with an Euler-pole term beside a target-sharded seismic wavemap (tests/test_gpu_eulerpole.py),
on 1 or 2 ranks: BEATAMD_TEST_MODE = "replicated" (one rank, the whole model) or "targets"
(beat_amd.models.sharded: the geodetic composite, with its pole term and the derived-coefficient buffer, is
replicated).  Two ranks share the one GPU through gloo.  Rank 0 writes the likelihood vectors of a population -- and,
replicated, those of the same model without corrections."""
import os
import sys
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist

    import beat_amd
    from beat_amd import parallel
    from beat_amd.models import EarthModel, EulerPoleConfig, ParameterLayout
    from beat_amd.models.sharded import TargetShardedLogp
    from beat_amd.synthetic import SyntheticSpec, build_problem, draw_population

    world = int(os.environ.get("WORLD_SIZE", "1"))
    mode = os.environ.get("BEATAMD_TEST_MODE", "replicated")
    torch.cuda.set_device(0)
    rank = 0
    if world > 1:
        os.environ["LOCAL_RANK"] = "0"
        rank, world, _ = parallel.init("gloo")
    dev = torch.device("cuda", 0)
    ctx = beat_amd.get_context(0)
    spec = SyntheticSpec((5,), (5,), (1.0,), T=5, N=96, D=3, S=25, covariance="toeplitz",
                         slip_varnames=("uparr", "uperp"), station_shifts=True, geodetic_nobs=(20, 31), laplacian=True,
                         interpolation="multilinear")
    prob, host = build_problem(spec)
    lay0 = host["layout"]
    rng = np.random.default_rng(43)
    n = spec.geodetic_nobs[1]
    los = rng.normal(size=(n, 3))
    mask = np.zeros(n, dtype=bool)
    mask[[3, 4, 5]] = True
    c = EulerPoleConfig(dataset_names=["scene_1"], enabled=True).init_correction()
    c.setup_correction(rng.uniform(36.0, 40.0, n), rng.uniform(20.0, 26.0, n), los, mask, "scene_1", number=1,
                       earth=EarthModel(6371.0e3, 6378.14e3, 1 / 298.257223563))
    corrs = [[], [c]]
    cnames = c.correction_names
    # the correction variables behind the others: every existing offset stays where it is
    prob.layout = ParameterLayout(OrderedDict(list(lay0.varsizes.items()) + [(k, 1) for k in cnames]))
    Q0 = draw_population(spec, lay0, host["lower"], host["upper"], 300)
    coef = rng.uniform(-1.0, 1.0, (300, 3)) * np.array([90.0, 180.0, 10.0])
    Q = torch.from_numpy(np.ascontiguousarray(np.hstack([Q0, coef]))).to(dev)
    extra = {}
    if mode == "replicated":
        f0 = prob.compile(ctx)
        extra["LL_plain"] = f0.batch(Q).cpu().numpy()
        f0.release()
    prob.geodetic.corrections = corrs
    f = TargetShardedLogp(prob, ctx) if mode == "targets" else prob.compile(ctx)
    if mode == "targets":
        assert f.world == world and f.nllk == spec.T + 2 + 1 + 1
    LL = f.batch(Q)
    ctx.synchronize()
    if rank == 0:
        np.savez(os.environ["BEATAMD_TEST_OUT"], LL=LL.cpu().numpy(), **extra)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print("SHARD_POLE_WORKER_OK rank", rank, flush=True)


if __name__ == "__main__":
    main()
