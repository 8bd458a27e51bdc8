"""Parallel tempering with proposal adaptation on 1 or 2 ranks (tests/test_gpu_ptadapt.py).

BEATAMD_TEST_BACKEND=gloo (default): every rank uses cuda:0 -- two ranks share ONE GPU, the collectives go through host
memory (beat_amd.parallel._staged).  2 posterior + 4 tempered temperatures x 8 replicas: two ranks hold three temperatures
each, so every temperature's window lives on one rank and no collective is needed for the proposals
(reference semantics: beat/sampler/pt.py:758-761, beat/sampler/base.py:363-393).  Rank 0 writes the samples, the manager's
history, the update steps and all ranks' proposal factors to BEATAMD_TEST_OUT."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_POST, N_TEMP, N_REPL = 2, 4, 8
SIGMA, H_BOX = 50.0, 0.01


def build(ctx):
    from beat_amd.synthetic import SyntheticSpec, build_problem
    # noise far above the synthetics and the noise-scaling hyper-parameter held to a narrow box: a soft likelihood, so that
    # the chains move and a window's weights spread over many samples.  (With the default noise, or h free in [-2, 2], one
    # state carries most of a window's weight: its covariance is rank deficient and goes through the host repair.)  2 x 2
    # patches, 16 parameters: a window of 40 steps x 8 replicas holds as many distinct states as moves were accepted, and
    # these must outnumber the parameters.  Dense (Toeplitz) data covariances, as in tests/_dist_gpu_worker.py: their
    # likelihoods do not depend on how the chains are cut into batches, to the last bit, which the comparison of one
    # rank with two needs (the weights of a window are exp(like)).
    spec = SyntheticSpec((2,), (2,), (1.0,), T=3, N=32, D=3, S=25, sigma=SIGMA, covariance="toeplitz")
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    lower, upper = dict(host["lower"]), dict(host["upper"])
    hyper = [k for k in host["layout"].varsizes if k.startswith("h_")]
    assert len(hyper) == 1
    lower[hyper[0]], upper[hyper[0]] = -H_BOX, H_BOX
    lo, up = host["layout"].bounds(lower, upper)
    return f, lo, up


def run_pt(f, lo, up, dev, **kw):
    """the run all comparisons share -> (samples, likelihoods, manager)"""
    from beat_amd.sampler import pt_sample
    span = np.where(up > lo, up - lo, 1.0)
    args = dict(n_chains_posterior=N_POST, n_chains_tempered=N_TEMP, n_replicas=N_REPL, n_samples=16 * 10,
                swap_interval=(10, 15), beta_tune_interval=3, proposal_cov=np.diag((0.01 * span) ** 2), device=dev,
                random_seed=5, tune_interval=20, update_proposal=True, buffer_size=40, burnin=30)
    args.update(kw)
    return pt_sample(f, lo, up, **args)


def main():
    import torch
    import torch.distributed as dist

    import beat_amd
    from beat_amd import parallel

    world = int(os.environ.get("WORLD_SIZE", "1"))
    backend = os.environ.get("BEATAMD_TEST_BACKEND", "gloo")
    local = int(os.environ.get("LOCAL_RANK", "0")) if backend == "nccl" else 0
    torch.cuda.set_device(local)
    rank = 0
    if world > 1:
        os.environ["LOCAL_RANK"] = str(local)
        rank, world, _ = parallel.init(backend)
    dev = torch.device("cuda", local)
    f, lo, up = build(beat_amd.get_context(local))
    s, ls, man = run_pt(f, lo, up, dev)
    F = man.proposal_factors
    factors = parallel.allgather_rows(F.reshape(F.shape[0], -1).contiguous()).cpu().numpy()
    flags = np.array([fl for _, fl in man.proposal_updates])
    if rank == 0:
        np.savez(os.environ["BEATAMD_TEST_OUT"], s=s, ls=ls, history=np.asarray(man.history), factors=factors,
                 update_steps=np.array([st for st, _ in man.proposal_updates]), flags=flags, scale=man.current_scale)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print("PTADAPT_GPU_WORKER_OK rank", rank, flush=True)


if __name__ == "__main__":
    main()
