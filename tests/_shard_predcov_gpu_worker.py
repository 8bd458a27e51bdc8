"""The velocity-model prediction covariance update on a joint problem whose seismic wavemap is target-sharded
(tests/test_gpu_predcov.py), on 1 or 2 ranks: BEATAMD_TEST_MODE = "replicated" (one rank, the whole model) or "targets"
(beat_amd.models.sharded: every rank compiles the rows of its targets; the geodetic composite is replicated and every
rank installs the same new operators).  Two ranks share the one GPU through gloo.  Rank 0 writes the likelihood vectors of
a population before and after the update.  ``joint_problem`` / ``crust_ensemble`` also serve the sampler test."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def joint_problem():
    """a small joint FFI problem: 5 targets of 96 samples with dense (Toeplitz) operators, two geodetic datasets of 20 and
    31 points, two slip variables -> (spec, problem, host arrays, the geodetic datasets' Covariance objects)"""
    from beat_amd.heart import Covariance
    from beat_amd.synthetic import SyntheticSpec, build_problem
    spec = SyntheticSpec((5,), (5,), (1.0,), T=5, N=96, D=3, S=25, covariance="toeplitz", slip_varnames=("uparr", "uperp"),
                         station_shifts=True, geodetic_nobs=(20, 31), interpolation="multilinear")
    prob, host = build_problem(spec)
    covs = []
    for W in host["gW"]:
        C = np.linalg.inv(W.T @ W)
        covs.append(Covariance(data=0.5 * (C + C.T)))
    return spec, prob, host, covs


def crust_ensemble(gfs, varnames, K, seed=7, spread=0.05):
    """K crust variants around the libraries ``gfs`` {varname: GeodeticGFLibrary}: variant 0 holds the same numbers as the
    model's own libraries, the others G (1 + spread N(0, 1)), seeded"""
    from beat_amd.ffi import GeodeticGFEnsemble, GeodeticGFLibrary, GeodeticGFLibraryConfig
    rng = np.random.default_rng(seed)
    libs = {}
    for k in range(K):
        libs[k] = {}
        for v in varnames:
            G = np.asarray(gfs[v].get_all())
            gf = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=G.shape, component=v, crust_ind=k))
            gf.setup(G.shape[0], G.shape[1], allocate=True)
            gf._gfmatrix[:] = G if k == 0 else G * (1.0 + spread * rng.standard_normal(G.shape))
            libs[k][v] = gf
    return GeodeticGFEnsemble(libs, varnames)


def main():
    import torch
    import torch.distributed as dist

    import beat_amd
    from beat_amd import parallel
    from beat_amd.covariance import VelocityModelCovarianceUpdate
    from beat_amd.models.sharded import TargetShardedLogp
    from beat_amd.synthetic import draw_population

    world = int(os.environ.get("WORLD_SIZE", "1"))
    mode = os.environ.get("BEATAMD_TEST_MODE", "replicated")
    torch.cuda.set_device(0)
    rank = 0
    if world > 1:
        os.environ["LOCAL_RANK"] = "0"
        rank, world, _ = parallel.init("gloo")
    dev = torch.device("cuda", 0)
    ctx = beat_amd.get_context(0)
    spec, prob, host, covs = joint_problem()
    Qh = draw_population(spec, host["layout"], host["lower"], host["upper"], 70)
    Q = torch.from_numpy(Qh).to(dev)
    f = TargetShardedLogp(prob, ctx) if mode == "targets" else prob.compile(ctx)
    before = f.batch(Q).cpu().numpy()
    upd = VelocityModelCovarianceUpdate(f, crust_ensemble(prob.geodetic.gfs, spec.slip_varnames, 6), covs)
    upd.update_weights(Qh[3])
    assert upd.n_updates == 1 and upd.n_host_route == 0
    after = f.batch(Q).cpu().numpy()
    ctx.synchronize()
    if rank == 0:
        np.savez(os.environ["BEATAMD_TEST_OUT"], before=before, after=after)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print("SHARD_PREDCOV_WORKER_OK rank", rank, flush=True)


if __name__ == "__main__":
    main()
