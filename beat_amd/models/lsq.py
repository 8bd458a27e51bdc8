"""
Start populations from non-negative least-squares slip -- the reference's ``initialization: lsq`` of the finite-fault
mode (beat/config.py:1121-1126).

There ``models/base.py:216-231`` draws one random point per chain and replaces its slip by
``DistributionOptimizer.lsq_solution(point)`` (models/problems.py:753-873): the non-negative least-squares solution of the
problem that is linear in the slip once the point's rupture kinematics are fixed.  The list of points is the ``start=`` of
``smc_sample`` / ``pt_sample`` / ``metropolis_sample``.  Here the points are the rows of one array and the solutions of all
chains come from one device call (``LogpForwFunc.lsq_solution``, csrc/lsq.hip):

    start = lsq_start_population(f, n_chains, random_seed)
    step = SMC(f, lower, upper, n_chains=n_chains, random_seed=random_seed)
    smc_sample(n_steps, step, start=start)

The prior points are drawn exactly as ``SMC.initialize_population`` draws them (same ``RandomState`` stream, same
expression), so every column that the solution does not replace equals the random start of that seed bit for bit.  The
slip is not clipped to the prior box (nor is the reference's): a component above the upper slip bound starts its chain
outside the box, where the Metropolis step leaves it only by an accepted move.
"""
import numpy as np

from .. import parallel


def prior_population(lower, upper, n_chains, random_seed):
    """the prior draws of ``SMC.initialize_population`` (metropolis.py:125-152) for all chains, on the host"""
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    rng = np.random.RandomState(random_seed)
    u = rng.random_sample((int(n_chains), lower.size))
    return lower + (upper - lower) * u


def lsq_start_population(f, n_chains, random_seed, lower=None, upper=None):
    """(n_chains, nparams) start array: prior draws whose slip is the non-negative least-squares solution at the draw's
    kinematics.  f: the compiled replicated model (``FFIProblem.compile``); lower / upper: the flat prior box (default: the
    problem's).  With several ranks each rank solves its block of chains (``parallel.chain_block``) and the blocks are
    all-gathered; a chain's solution does not depend on the batch it is solved in, so the array is the one a single rank
    computes, bit for bit.  Errors are those of ``LogpForwFunc.lsq_solution``."""
    if not hasattr(f, "problem") or not hasattr(f, "lsq_solution"):
        raise TypeError("lsq_start_population needs a compiled FFI model")
    from .problem import refuse_polarity, refuse_spectrum_wavemaps
    refuse_spectrum_wavemaps(f.problem, "the least-squares start")      # (not linear in the slips; before anything is drawn)
    refuse_polarity(f.problem, "lsq_start_population")
    if lower is None or upper is None:
        prob = f.problem
        if prob.lower is None or prob.upper is None:
            raise ValueError("the problem holds no prior box: pass lower and upper")
        lower, upper = prob.layout.bounds(prob.lower, prob.upper)
    pop = prior_population(lower, upper, n_chains, random_seed)
    if pop.shape[1] != f.nparams:
        raise ValueError("the prior box has %d parameters, the model %d" % (pop.shape[1], f.nparams))
    rank, world, _ = parallel.ensure_group()
    if world == 1:
        return f.lsq_solution(pop)
    import torch
    a, b = parallel.chain_block(int(n_chains), rank, world)
    local = f.lsq_solution(np.ascontiguousarray(pop[a:b]))
    dev = torch.device("cuda", f.ctx.device)
    return parallel.allgather_rows(torch.from_numpy(local).to(dev), int(n_chains)).cpu().numpy()
