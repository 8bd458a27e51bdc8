"""The least-squares start on 1 or more ranks that share cuda:0 (tests/test_gpu_lsq.py; gloo transport, as
tests/_dist_gpu_worker.py): every rank solves its block of chains, the gathered start population and the SMC run from it
are written by rank 0 to BEATAMD_TEST_OUT; the test compares the files of a 1-rank and a 2-rank run bit for bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import torch.distributed as dist

    import beat_amd
    import lsq_ref
    from beat_amd import parallel
    from beat_amd.models.lsq import lsq_start_population
    from beat_amd.sampler import SMC, smc_sample

    world = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0)
    rank = 0
    if world > 1:
        os.environ["LOCAL_RANK"] = "0"
        rank, world, _ = parallel.init("gloo")
    dev = torch.device("cuda", 0)
    ctx = beat_amd.get_context(0)
    case = lsq_ref.load_case(np.load(os.path.join(ROOT, "tests", "golden", "lsq.npz")), "joint3x4")
    prob, lay = lsq_ref.build_problem(case)
    f = prob.compile(ctx)
    lo, up = case["lower"], case["upper"]
    n = 96
    start = lsq_start_population(f, n, 13)
    step = SMC(f, lo, up, n_chains=n, device=dev, random_seed=13, tune_interval=3)
    assert step.block == parallel.chain_block(n, rank, world)
    pop, lp, betas = smc_sample(3, step, max_stages=2, start=start)
    if rank == 0:
        np.savez(os.environ["BEATAMD_TEST_OUT"], start=start, pop=pop, lp=lp, betas=np.asarray(betas))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print("LSQ_GPU_WORKER_OK rank", rank, flush=True)


if __name__ == "__main__":
    main()
