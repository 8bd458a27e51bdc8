"""Device SMC of a polarity problem on 1 or more ranks (tests/test_gpu_polarity.py): every rank uses cuda:0 -- two ranks
share ONE GPU, the collectives go through host memory (gloo).  Rank 0 writes population, likelihoods and betas to
BEATAMD_TEST_OUT; the test compares the files of a 1-rank and a 2-rank run bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def main():
    import torch
    import torch.distributed as dist

    import beat_amd
    import test_gpu_polarity as tp
    from beat_amd import parallel
    from beat_amd.sampler import SMC, smc_sample

    os.environ["BEATAMD_CHECK_RANKS"] = "1"   # transition(): beta, weights, indices, factor bitwise equal on all ranks
    world = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0)
    rank = 0
    if world > 1:
        os.environ["LOCAL_RANK"] = "0"
        rank, world, _ = parallel.init("gloo")
    dev = torch.device("cuda", 0)
    ctx = beat_amd.get_context(0)
    prob, lay, lower, upper = tp._model("mtqt", 65, 41)
    f = prob.compile(ctx)
    lo, up = lay.bounds(lower, upper)
    step = SMC(f, lo, up, n_chains=256, device=dev, random_seed=11, tune_interval=3)
    assert step.block == parallel.chain_block(256, rank, world)
    pop, lp, betas = smc_sample(4, step, max_stages=3)
    if rank == 0:
        np.savez(os.environ["BEATAMD_TEST_OUT"], pop=pop, lp=lp, betas=np.asarray(betas))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print("POLARITY_GPU_WORKER_OK rank", rank, flush=True)


if __name__ == "__main__":
    main()
